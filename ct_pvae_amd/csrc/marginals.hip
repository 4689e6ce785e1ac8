// marginals.hip -- per-pixel marginals of the TruncatedNormal output head (the reference's CT_VAE.pixel_dist, ctvae/main_ct_vae.py:648-731):
// for decoder outputs alpha, beta [n][pix] and K draws, the histogram, the sum and the sum of squares of the n * K samples of every
// pixel, accumulated into caller-owned state.  No sample is written to memory: it is drawn, binned and added in registers / LDS.
//
// Sample (o, pixel, k) IS the x that ctpvae_tn_head_fwd_f32 writes for object o and that pixel with draw = draw0 + k and the same seed
// and first_object: tn_head.h's tn_prep / tn_draw on the uniform of head_uniforms4 (word e & 3 of the block of e = (first_object + o) *
// pix + pixel), the code head.hip runs.  The lp terms are not evaluated.
//
// Bin of a sample, fp32 (marginals_bin, host and device; ctpvae_tn_marginals_bin_host_f32 applies it to an array):
//   t = (x - lo) / width         one subtraction, one correctly rounded division
//   column 0 if !(t >= 0) (NaN too), column bins + 1 if t >= bins, else column 1 + (int)t
//
// State: hist [pix][bins + 2] int64, s1, s2 [pix] float64 (sum of the samples and of their squares, each fp32 sample widened to double
// first; the square of a float is exact in double).  All n objects add into the same pix rows.  A launch ADDS to the state.
//
// Layout.  The draws 0 .. K-1 are cut into S = ceil(K / 25) slices of kMargSlice = 25 consecutive draws (the last may be shorter; 25
// divides the reference's 100 draws per decoder output).  Unit j = o * S + s is slice s of object o, n * S units in all.  A workgroup
// of 256 threads covers a tile of 16 quads = 64 pixels (grid x) and has 16 unit lanes: thread t = 16 * lane + quad.  There are
// G = min(ceil(n * S / 16), kMargMaxGroups = 64) workgroups per tile (grid y); lane l of group g takes the units
//   j = 16 g + l,  16 (g + G) + l,  16 (g + 2 G) + l, ...                                       (ascending)
// and walks the draws of each ascending.  Per unit it loads its quad of alpha, beta and evaluates tn_prep once (so the part that
// does not depend on u is evaluated once per pixel, object and slice of 25 draws, not once per sample); per draw it takes one Philox
// block for the quad when the quad is whole-block aligned ((first_object + o) * pix a multiple of 4), two otherwise.
//
// Counts: one LDS add per sample into the workgroup's [64][bins + 2] 32-bit image (n * K < 2^32, so it cannot wrap), then at most one
// 64-bit integer atomic add per pixel, column and workgroup into hist, zeros skipped.  Integer addition commutes: any order, same bits.
//
// The float64 sums, in this fixed order and with no floating-point atomics (s1 shown; s2 alike with the squares):
//   thread (g, l), pixel p:  P_gl = (((0 + x_1) + x_2) + ...)      its samples of p in the order it draws them (units ascending as
//                                                                  above, draws ascending inside a unit); a thread without samples: 0
//   workgroup g:             W_g  = ((P_g0 + P_g1) + ...) + P_g15  lanes ascending, through LDS
//   launch:                  T    = ((W_0 + W_1) + ...) + W_(G-1)  groups ascending, by a second kernel from the workspace [G][2][pix]
//   state:                   s1[p] = s1[p] + T
// The workspace is G * 2 * pix doubles: at most 64 * 16 * pix bytes whatever K is.
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

__global__ __launch_bounds__(kMargThreads) void tn_marginals_kernel(const float *__restrict__ alpha, const float *__restrict__ beta,
                                                                    MargShape sh, int ptr_aligned, unsigned long long *__restrict__ hist,
                                                                    double *__restrict__ ws)
{
    extern __shared__ __align__(16) unsigned char marg_lds[];
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
            TnPrep pr[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) pr[q] = tn_prep(al[q], be[q]);
            const unsigned kb = s * kMargSlice;
            const unsigned ke = sh.draws - kb < kMargSlice ? sh.draws : kb + kMargSlice;
            for (unsigned k = kb; k < ke; ++k) {
                float u[4];
                head_uniforms4(sh.first_pixel + i, sh.draw0 + k, sh.k0, sh.k1, u);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float x = tn_draw(pr[q], u[q]).x;
                    if (q < cnt) {
                        atomicAdd(row + q * cols + marginals_bin(x, sh.lo, sh.width, sh.bins), 1u);
                        const double xd = (double)x;
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

// s1[p] += T, s2[p] += T' with T the ascending sum of the launch's G workgroup partials
__global__ __launch_bounds__(kMargThreads) void tn_marginals_finish_kernel(const double *__restrict__ ws, int pix, int groups,
                                                                           double *__restrict__ s1, double *__restrict__ s2)
{
    const size_t i = (size_t)blockIdx.x * kMargThreads + threadIdx.x;   // [2][pix]
    if (i >= 2 * (size_t)pix) return;
    double tot = ws[i];
    for (int g = 1; g < groups; ++g) tot += ws[(size_t)g * 2 * pix + i];
    double *dst = i < (size_t)pix ? s1 + i : s2 + (i - pix);
    *dst = *dst + tot;
}

static int marg_check(const char *what, int n, int pix, unsigned draws)
{
    CTPVAE_REQUIRE(n > 0 && pix > 0, "%s: sizes must be positive (n=%d pix=%d)", what, n, pix);
    CTPVAE_REQUIRE((long long)n * pix <= INT_MAX, "%s: n * pix must fit 31 bits (n=%d pix=%d)", what, n, pix);
    CTPVAE_REQUIRE(draws >= 1, "%s: draws must be >= 1", what);
    CTPVAE_REQUIRE((unsigned long long)n * draws <= UINT_MAX, "%s: n * draws must fit 32 bits (n=%d draws=%u)", what, n, draws);
    return CTPVAE_OK;
}

static int marg_grid_check(const char *what, float lo, float width, int bins)
{
    CTPVAE_REQUIRE(bins >= 1 && bins <= CTPVAE_MARGINALS_MAX_BINS, "%s: bins must be 1 .. %d (got %d)", what, CTPVAE_MARGINALS_MAX_BINS, bins);
    CTPVAE_REQUIRE(std::isfinite(lo) && std::isfinite(width) && width > 0.0f, "%s: lo and width must be finite, width > 0 (got %g, %g)",
                   what, (double)lo, (double)width);
    return CTPVAE_OK;
}

}  // namespace ctpvae

using namespace ctpvae;

extern "C" {

long long ctpvae_tn_marginals_workspace_bytes(int n, int pix, unsigned draws)
{
    if (int rc = marg_check("tn_marginals_workspace_bytes", n, pix, draws)) return rc;
    return (long long)marg_groups(n, draws) * 2 * pix * (long long)sizeof(double);
}

int ctpvae_tn_marginals_f32(const float *alpha_dev, const float *beta_dev, int n, int pix, long long first_object,
                            unsigned long long seed, unsigned draw0, unsigned draws, float lo, float width, int bins,
                            long long *hist_dev, double *s1_dev, double *s2_dev, void *workspace_dev, ctpvae_stream_t stream)
{
    static std::atomic<unsigned long long> attr_set{0};
    if (int rc = head_check("tn_marginals", alpha_dev, beta_dev, n, pix, first_object)) return rc;
    if (int rc = marg_check("tn_marginals", n, pix, draws)) return rc;
    if (int rc = marg_grid_check("tn_marginals", lo, width, bins)) return rc;
    CTPVAE_REQUIRE((unsigned long long)draw0 + draws <= (1ull << 32), "tn_marginals: draw0 + draws must be <= 2^32 (got %u + %u)", draw0,
                   draws);
    CTPVAE_REQUIRE(hist_dev && s1_dev && s2_dev && workspace_dev, "tn_marginals: null state or workspace pointer");
    CTPVAE_REQUIRE(((size_t)hist_dev & 7) == 0 && ((size_t)s1_dev & 7) == 0 && ((size_t)s2_dev & 7) == 0 && ((size_t)workspace_dev & 7) == 0,
                   "tn_marginals: state and workspace must be 8-byte aligned");
    MargShape sh;
    sh.n = n, sh.pix = pix, sh.bins = bins, sh.groups = marg_groups(n, draws);
    sh.draws = draws, sh.slices = marg_slices(draws), sh.units = (unsigned)n * sh.slices;
    sh.first_pixel = (unsigned long long)first_object * (unsigned long long)pix;
    sh.draw0 = draw0, sh.k0 = (unsigned)seed, sh.k1 = (unsigned)(seed >> 32);
    sh.lo = lo, sh.width = width;
    const int aligned = head_aligned16({alpha_dev, beta_dev}) ? 1 : 0;
    const int tiles = ceil_div(pix, kMargTilePix);
    const size_t lds = (size_t)kMargMomBytes + (size_t)kMargTilePix * (bins + 2) * sizeof(unsigned);   // <= 80 KiB
    CTPVAE_SET_MAX_LDS_ONCE(tn_marginals_kernel, attr_set);
    hipLaunchKernelGGL(tn_marginals_kernel, dim3(tiles, sh.groups), dim3(kMargThreads), lds, (hipStream_t)stream, alpha_dev, beta_dev, sh,
                       aligned, reinterpret_cast<unsigned long long *>(hist_dev), static_cast<double *>(workspace_dev));
    CTPVAE_LAUNCH_CHECK("tn_marginals_kernel");
    hipLaunchKernelGGL(tn_marginals_finish_kernel, dim3((unsigned)((2ll * pix + kMargThreads - 1) / kMargThreads)), dim3(kMargThreads), 0, (hipStream_t)stream,
                       static_cast<const double *>(workspace_dev), pix, sh.groups, s1_dev, s2_dev);
    CTPVAE_LAUNCH_CHECK("tn_marginals_finish_kernel");
    return CTPVAE_OK;
}

int ctpvae_tn_marginals_bin_host_f32(const float *x_host, long long count, float lo, float width, int bins, int *col_out_host)
{
    CTPVAE_REQUIRE(x_host && col_out_host, "tn_marginals_bin_host: null pointer");
    CTPVAE_REQUIRE(count >= 0, "tn_marginals_bin_host: count must be >= 0 (got %lld)", count);
    if (int rc = marg_grid_check("tn_marginals_bin_host", lo, width, bins)) return rc;
    for (long long i = 0; i < count; ++i) col_out_host[i] = marginals_bin(x_host[i], lo, width, bins);
    return CTPVAE_OK;
}

}  // extern "C"
