// marginals.h -- what marginals.hip (per-pixel marginals of the TruncatedNormal head's samples) and beta_marginals.hip (of the Beta
// head's) share: the bin rule, the cut of the draws into units, the launch shape, the workgroup's walk over its units with the counts
// and the float64 sums in their fixed order, the finishing step and the argument checks.  marginals.hip's header states all of it; a
// file adds only its sampler (what a thread evaluates once per unit, and the four samples of a quad for one draw) and its two kernels,
// so both heads' marginals bin, count and add alike.
#pragma once
#include <cmath>

#include "tn_head.h"

namespace ctpvae {

constexpr int kMargThreads = 256;
constexpr int kMargTileQuads = 16;                              // quads of a workgroup's tile
constexpr int kMargTilePix = 4 * kMargTileQuads;                // 64 pixels
constexpr int kMargLanes = kMargThreads / kMargTileQuads;       // 16 unit lanes
constexpr unsigned kMargSlice = 25;                             // draws per unit
constexpr int kMargMaxGroups = 64;                              // workgroups per tile at most
constexpr int kMargMomBytes = 2 * kMargLanes * kMargTilePix * (int)sizeof(double);   // the lanes' partial sums in LDS: 16 KiB

__host__ __device__ inline int marginals_bin(float x, float lo, float width, int bins)
{
    const float t = (x - lo) / width;
    if (!(t >= 0.0f)) return 0;
    if (t >= (float)bins) return bins + 1;
    return 1 + (int)t;
}

struct MargShape {
    int n, pix, bins, groups;
    unsigned draws, slices, units;    // K, S, n * S
    unsigned long long first_pixel;   // first_object * pix
    unsigned draw0, k0, k1;
    float lo, width;
};

inline unsigned marg_slices(unsigned draws) { return draws / kMargSlice + (draws % kMargSlice != 0 ? 1u : 0u); }   // (draws + 24 may wrap)
inline int marg_groups(int n, unsigned draws)
{
    const unsigned long long units = (unsigned long long)n * marg_slices(draws);
    const unsigned long long g = (units + kMargLanes - 1) / kMargLanes;
    return g < (unsigned long long)kMargMaxGroups ? (int)g : kMargMaxGroups;
}

inline size_t marg_lds_bytes(int bins) { return (size_t)kMargMomBytes + (size_t)kMargTilePix * (bins + 2) * sizeof(unsigned); }   // <= 80 KiB

// One workgroup's work (marginals.hip's header: layout, counts, the order of the sums).  A Sampler has
//   void prep(const float (&al)[4], const float (&be)[4])          once per unit: what does not depend on the random numbers
//   void draw(unsigned long long e, unsigned draw, unsigned k0, unsigned k1, int cnt, float (&x)[4])
//                                                                  the samples of the quad's first cnt pixels, e the flat index of
//                                                                  its first pixel (x[q], q >= cnt, is not read)
template <class Sampler>
__device__ __forceinline__ void marg_workgroup(const float *__restrict__ alpha, const float *__restrict__ beta, const MargShape &sh,
                                               int ptr_aligned, unsigned long long *__restrict__ hist, double *__restrict__ ws,
                                               unsigned char *marg_lds)
{
    double *mom = reinterpret_cast<double *>(marg_lds);                            // [2][lanes][64]
    unsigned *cnt_img = reinterpret_cast<unsigned *>(marg_lds + kMargMomBytes);    // [64][cols]
    const int t = threadIdx.x, ql = t & (kMargTileQuads - 1), lane = t >> 4;
    const int cols = sh.bins + 2;
    const int tile0 = blockIdx.x * kMargTilePix;              // first pixel of the tile
    for (int i = t; i < kMargTilePix * cols; i += kMargThreads) cnt_img[i] = 0u;
    __syncthreads();

    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    const int r = tile0 + 4 * ql;                             // first pixel of this thread's quad
    if (r < sh.pix) {
        const int cnt = sh.pix - r < 4 ? sh.pix - r : 4;
        unsigned *row = cnt_img + 4 * ql * cols;
        const unsigned stride = (unsigned)sh.groups * kMargLanes;
        // units < 2^32 and stride <= 1024: the 64-bit counter only keeps the last step from wrapping
        for (unsigned long long jj = (unsigned)blockIdx.y * kMargLanes + lane; jj < sh.units; jj += stride) {
            const unsigned j = (unsigned)jj;
            const unsigned o = j / sh.slices, s = j - o * sh.slices;
            const size_t base = (size_t)o * sh.pix;
            const size_t i = base + r;
            const bool vec = ptr_aligned != 0 && (base & 3) == 0;
            float al[4], be[4];
            quad_load(alpha, i, cnt, vec, 1.0f, al);
            quad_load(beta, i, cnt, vec, 1.0f, be);
            Sampler smp;
            smp.prep(al, be);
            const unsigned kb = s * kMargSlice;
            const unsigned ke = sh.draws - kb < kMargSlice ? sh.draws : kb + kMargSlice;
            for (unsigned k = kb; k < ke; ++k) {
                float x[4];
                smp.draw(sh.first_pixel + i, sh.draw0 + k, sh.k0, sh.k1, cnt, x);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (q < cnt) {
                        atomicAdd(row + q * cols + marginals_bin(x[q], sh.lo, sh.width, sh.bins), 1u);
                        const double xd = (double)x[q];
                        s1[q] += xd;
                        s2[q] += xd * xd;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        mom[lane * kMargTilePix + 4 * ql + q] = s1[q];
        mom[(kMargLanes + lane) * kMargTilePix + 4 * ql + q] = s2[q];
    }
    __syncthreads();

    // counts: this workgroup's rows of hist are contiguous, [tile0 .. tile0 + 64) x cols
    const int live = (sh.pix - tile0 < kMargTilePix ? sh.pix - tile0 : kMargTilePix) * cols;
    unsigned long long *hist_tile = hist + (size_t)tile0 * cols;
    for (int i = t; i < live; i += kMargThreads) {
        const unsigned c = cnt_img[i];
        if (c != 0u) atomicAdd(hist_tile + i, (unsigned long long)c);
    }
    // moments: W_g of each of the tile's pixels, lanes ascending
    if (t < 2 * kMargTilePix) {
        const int p = t & (kMargTilePix - 1), which = t >> 6;
        const double *m = mom + which * kMargLanes * kMargTilePix + p;
        double acc = m[0];
#pragma unroll
        for (int l = 1; l < kMargLanes; ++l) acc += m[l * kMargTilePix];
        if (tile0 + p < sh.pix) ws[((size_t)blockIdx.y * 2 + which) * sh.pix + tile0 + p] = acc;
    }
}

// the finishing step: s1[p] += T, s2[p] += T' with T the ascending sum of the launch's G workgroup partials
__device__ __forceinline__ void marg_finish(const double *__restrict__ ws, int pix, int groups, double *__restrict__ s1,
                                            double *__restrict__ s2)
{
    const size_t i = (size_t)blockIdx.x * kMargThreads + threadIdx.x;   // [2][pix]
    if (i >= 2 * (size_t)pix) return;
    double tot = ws[i];
    for (int g = 1; g < groups; ++g) tot += ws[(size_t)g * 2 * pix + i];
    double *dst = i < (size_t)pix ? s1 + i : s2 + (i - pix);
    *dst = *dst + tot;
}

inline unsigned marg_finish_blocks(int pix) { return (unsigned)((2ll * pix + kMargThreads - 1) / kMargThreads); }

inline int marg_check(const char *what, int n, int pix, unsigned draws)
{
    CTPVAE_REQUIRE(n > 0 && pix > 0, "%s: sizes must be positive (n=%d pix=%d)", what, n, pix);
    CTPVAE_REQUIRE((long long)n * pix <= INT_MAX, "%s: n * pix must fit 31 bits (n=%d pix=%d)", what, n, pix);
    CTPVAE_REQUIRE(draws >= 1, "%s: draws must be >= 1", what);
    CTPVAE_REQUIRE((unsigned long long)n * draws <= UINT_MAX, "%s: n * draws must fit 32 bits (n=%d draws=%u)", what, n, draws);
    return CTPVAE_OK;
}

inline int marg_grid_check(const char *what, float lo, float width, int bins)
{
    CTPVAE_REQUIRE(bins >= 1 && bins <= CTPVAE_MARGINALS_MAX_BINS, "%s: bins must be 1 .. %d (got %d)", what, CTPVAE_MARGINALS_MAX_BINS, bins);
    CTPVAE_REQUIRE(std::isfinite(lo) && std::isfinite(width) && width > 0.0f, "%s: lo and width must be finite, width > 0 (got %g, %g)",
                   what, (double)lo, (double)width);
    return CTPVAE_OK;
}

// every check of a marginals launch, in one order for both heads (nothing is launched before all of them pass), then its shape
inline int marg_launch_shape(const char *what, const float *alpha_dev, const float *beta_dev, int n, int pix, long long first_object,
                             unsigned long long seed, unsigned draw0, unsigned draws, float lo, float width, int bins,
                             const void *hist_dev, const void *s1_dev, const void *s2_dev, const void *workspace_dev, MargShape &sh)
{
    if (int rc = head_check(what, alpha_dev, beta_dev, n, pix, first_object)) return rc;
    if (int rc = marg_check(what, n, pix, draws)) return rc;
    if (int rc = marg_grid_check(what, lo, width, bins)) return rc;
    CTPVAE_REQUIRE((unsigned long long)draw0 + draws <= (1ull << 32), "%s: draw0 + draws must be <= 2^32 (got %u + %u)", what, draw0, draws);
    CTPVAE_REQUIRE(hist_dev && s1_dev && s2_dev && workspace_dev, "%s: null state or workspace pointer", what);
    CTPVAE_REQUIRE(((size_t)hist_dev & 7) == 0 && ((size_t)s1_dev & 7) == 0 && ((size_t)s2_dev & 7) == 0 && ((size_t)workspace_dev & 7) == 0,
                   "%s: state and workspace must be 8-byte aligned", what);
    sh.n = n, sh.pix = pix, sh.bins = bins, sh.groups = marg_groups(n, draws);
    sh.draws = draws, sh.slices = marg_slices(draws), sh.units = (unsigned)n * sh.slices;
    sh.first_pixel = (unsigned long long)first_object * (unsigned long long)pix;
    sh.draw0 = draw0, sh.k0 = (unsigned)seed, sh.k1 = (unsigned)(seed >> 32);
    sh.lo = lo, sh.width = width;
    return CTPVAE_OK;
}

}  // namespace ctpvae
