// convblock.hip -- the glue around every convolution of the P-VAE's ConvBlock (ctvae/models.py:219-263, :330-341;
// ct_pvae_amd/trainer.py _PeriodicPad and _Maxout) as ONE launch each way: the 'periodic' padding of the two spatial axes and the
// maxout of the two channel halves.  All four kernels are pure streaming on contiguous fp32 [N][C][H][W] tensors: no LDS, no atomics,
// no arithmetic but the backward's additions.
//
// Periodic pad, planes = N * C, pads (wl, wr, hl, hr) >= 0, OH = H + hl + hr, OW = W + wl + wr, mod the mathematical modulo (a pad may
// exceed the extent: at H = 1 every padded row is row 0):
//   forward    out[p][r][q] = x[p][(r - hl) mod H][(q - wl) mod W]                       r < OH, q < OW
//   backward   a deterministic gather, one thread per four source elements, in this order of addition:
//     t[r][j]  = the sum over q ASCENDING of g[p][r][q] with (q - wl) mod W = j          (q = q0, q0 + W, ...; q0 = (j + wl) mod W)
//     gx[p][i][j] = the sum over r ASCENDING of t[r][j] with (r - hl) mod H = i          (r = r0, r0 + H, ...; r0 = (i + hl) mod H)
//   each sum starts from its first term (no + 0.0f in front).  With at most two copies per axis this is the value of the
//   index_add_ chain of trainer._PeriodicPad; with more, only this order is defined.  The build's -ffp-contract=off keeps the
//   additions as written.
//
// Maxout, y [N][2C][H][W], len = C * H * W, a = y[n][i], b = y[n][len + i]:
//   forward    first = a >= b;  out[n][i] = first ? a : b;  first_out[n][i] = first (one byte, 0 or 1: all the backward needs)
//              a tie takes the first half (TensorFlow's MaximumGrad); a NaN in either half makes the comparison false and takes the
//              second half; -0.0 >= +0.0 is true
//   backward   gy[n][i] = first ? g : +0.0f;  gy[n][len + i] = first ? +0.0f : g -- a selection, not g * first: an infinite cotangent
//              gives (inf, 0), not (inf, NaN); every element of gy is written
//
// Layout: a thread moves a quad, four consecutive elements of the array it WRITES (the padded output, gx, out, gy), with one 16-byte
// store when the quad is whole and 16-byte aligned; what it reads comes with one 16-byte load when the four sources are consecutive
// in memory and 16-byte aligned, with guarded 4-byte loads otherwise (the padded width is odd for most layers, so a padded row
// rarely starts aligned).  256 threads per workgroup, at most 2048 workgroups, a grid-stride loop over the quads.  Every element
// count is below 2^31.
#include <climits>

#include "common.h"
#include "quad_io.h"

namespace ctpvae {

constexpr int kConvBlockThreads = 256;
constexpr unsigned kConvBlockMaxGrid = 2048;

struct PadGeom {
    int H, W, OH, OW;
    int sr0, sq0;   // source row / column of padded row / column 0: (-hl) mod H, (-wl) mod W
    int r0, q0;     // first padded row / column of source row / column 0: hl mod H, wl mod W
};

// out quad e .. e+3 of the flat padded array [planes][OH][OW]
__global__ __launch_bounds__(kConvBlockThreads) void periodic_pad_fwd_kernel(const float *__restrict__ x, float *__restrict__ out, PadGeom gm,
                                                                              unsigned total, int ptr_aligned)
{
    const unsigned quads = (total >> 2) + ((total & 3u) != 0);
    const bool al = ptr_aligned != 0;
    for (unsigned qd = blockIdx.x * kConvBlockThreads + threadIdx.x; qd < quads; qd += gridDim.x * kConvBlockThreads) {
        const unsigned e = 4u * qd;
        const int cnt = total - e < 4u ? (int)(total - e) : 4;
        const unsigned row = e / (unsigned)gm.OW;                  // p * OH + r
        int q = (int)(e - row * (unsigned)gm.OW);
        unsigned p = row / (unsigned)gm.OH;
        int r = (int)(row - p * (unsigned)gm.OH);
        int sr = (r + gm.sr0) % gm.H, sq = (q + gm.sq0) % gm.W;
        size_t src = ((size_t)p * gm.H + sr) * gm.W;               // the source row's first element
        float v[4];
        if (al && cnt == 4 && q + 3 < gm.OW && sq + 3 < gm.W && ((src + sq) & 3) == 0) {
            const float4 f = ld4(x + src + sq);
            v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = j < cnt ? x[src + sq] : 0.0f;
                if (++sq == gm.W) sq = 0;
                if (++q == gm.OW) {                                // the quad goes on in the next padded row
                    q = 0, sq = gm.sq0;
                    if (++r == gm.OH) r = 0, ++p, sr = gm.sr0;
                    else if (++sr == gm.H) sr = 0;
                    src = ((size_t)p * gm.H + sr) * gm.W;
                }
            }
        }
        quad_store(out, e, cnt, al, v);
    }
}

// one source element: the two ascending folds of the file header
__device__ __forceinline__ float pad_bwd_one(const float *__restrict__ g, const PadGeom &gm, unsigned p, int i, int j)
{
    int r = i + gm.r0, q0 = j + gm.q0;
    if (r >= gm.H) r -= gm.H;
    if (q0 >= gm.W) q0 -= gm.W;
    float acc = 0.0f;
    for (bool first = true; r < gm.OH; r += gm.H, first = false) {
        const size_t base = ((size_t)p * gm.OH + r) * gm.OW;
        float t = g[base + q0];
        for (int q = q0 + gm.W; q < gm.OW; q += gm.W) t += g[base + q];
        acc = first ? t : acc + t;
    }
    return acc;
}

// gx quad e .. e+3 of the flat source array [planes][H][W]
__global__ __launch_bounds__(kConvBlockThreads) void periodic_pad_bwd_kernel(const float *__restrict__ g, float *__restrict__ gx, PadGeom gm,
                                                                              unsigned total, int ptr_aligned)
{
    const unsigned quads = (total >> 2) + ((total & 3u) != 0);
    const bool al = ptr_aligned != 0;
    for (unsigned qd = blockIdx.x * kConvBlockThreads + threadIdx.x; qd < quads; qd += gridDim.x * kConvBlockThreads) {
        const unsigned e = 4u * qd;
        const int cnt = total - e < 4u ? (int)(total - e) : 4;
        const unsigned row = e / (unsigned)gm.W;                   // p * H + i
        int j = (int)(e - row * (unsigned)gm.W);
        unsigned p = row / (unsigned)gm.H;
        int i = (int)(row - p * (unsigned)gm.H);
        float acc[4];
        int q0 = j + gm.q0;
        if (q0 >= gm.W) q0 -= gm.W;
        if (cnt == 4 && j + 3 < gm.W && q0 + 3 < gm.W) {
            // the four elements share their padded rows and their copies are consecutive columns: quads of g, the same two folds
            int r = i + gm.r0;
            if (r >= gm.H) r -= gm.H;
            acc[0] = acc[1] = acc[2] = acc[3] = 0.0f;
            for (bool first = true; r < gm.OH; r += gm.H, first = false) {
                const size_t base = ((size_t)p * gm.OH + r) * gm.OW;
                float t[4];
                quad_load(g, base + q0, 4, al && ((base + q0) & 3) == 0, 0.0f, t);     // q0 + 3 < W <= OW: all four exist
                for (int q = q0 + gm.W; q < gm.OW; q += gm.W) {
                    const int n = gm.OW - q < 4 ? gm.OW - q : 4;                       // element k has this copy when q + k < OW
                    float u[4];
                    quad_load(g, base + q, n, al && ((base + q) & 3) == 0, 0.0f, u);
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < n) t[k] += u[k];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = first ? t[k] : acc[k] + t[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                acc[k] = k < cnt ? pad_bwd_one(g, gm, p, i, j) : 0.0f;
                if (++j == gm.W) {
                    j = 0;
                    if (++i == gm.H) i = 0, ++p;
                }
            }
        }
        quad_store(gx, e, cnt, al, acc);
    }
}

__global__ __launch_bounds__(kConvBlockThreads) void maxout_fwd_kernel(const float *__restrict__ y, int len, unsigned quads_per_object,
                                                                        unsigned quads, int ptr_aligned, float *__restrict__ out,
                                                                        unsigned char *__restrict__ first_out)
{
    const bool al = ptr_aligned != 0;
    const size_t L = (size_t)len;
    for (unsigned qd = blockIdx.x * kConvBlockThreads + threadIdx.x; qd < quads; qd += gridDim.x * kConvBlockThreads) {
        const unsigned n = qd / quads_per_object;
        const int r = 4 * (int)(qd - n * quads_per_object);
        const int cnt = len - r < 4 ? len - r : 4;
        const size_t a0 = 2 * (size_t)n * L + r, b0 = a0 + L, o0 = (size_t)n * L + r;
        float a[4], b[4], v[4];
        quad_load(y, a0, cnt, al && (a0 & 3) == 0, 0.0f, a);
        quad_load(y, b0, cnt, al && (b0 & 3) == 0, 0.0f, b);
        unsigned bits = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool first = a[k] >= b[k];
            v[k] = first ? a[k] : b[k];
            bits |= (first ? 1u : 0u) << (8 * k);
        }
        const bool vec_o = al && (o0 & 3) == 0;
        quad_store(out, o0, cnt, vec_o, v);
        if (vec_o && cnt == 4) {
            *reinterpret_cast<unsigned *>(first_out + o0) = bits;      // four bytes, little-endian: byte k is element k
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) first_out[o0 + k] = (unsigned char)((bits >> (8 * k)) & 1u);
        }
    }
}

__global__ __launch_bounds__(kConvBlockThreads) void maxout_bwd_kernel(const float *__restrict__ g, const unsigned char *__restrict__ first_in,
                                                                        int len, unsigned quads_per_object, unsigned quads, int ptr_aligned,
                                                                        float *__restrict__ gy)
{
    const bool al = ptr_aligned != 0;
    const size_t L = (size_t)len;
    for (unsigned qd = blockIdx.x * kConvBlockThreads + threadIdx.x; qd < quads; qd += gridDim.x * kConvBlockThreads) {
        const unsigned n = qd / quads_per_object;
        const int r = 4 * (int)(qd - n * quads_per_object);
        const int cnt = len - r < 4 ? len - r : 4;
        const size_t a0 = 2 * (size_t)n * L + r, b0 = a0 + L, o0 = (size_t)n * L + r;
        const bool vec_o = al && (o0 & 3) == 0;
        float gv[4], ga[4], gb[4];
        quad_load(g, o0, cnt, vec_o, 0.0f, gv);
        unsigned bits = 0;
        if (vec_o && cnt == 4) {
            bits = *reinterpret_cast<const unsigned *>(first_in + o0);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) bits |= (unsigned)first_in[o0 + k] << (8 * k);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool first = ((bits >> (8 * k)) & 0xFFu) != 0;
            ga[k] = first ? gv[k] : 0.0f;
            gb[k] = first ? 0.0f : gv[k];
        }
        quad_store(gy, a0, cnt, al && (a0 & 3) == 0, ga);
        quad_store(gy, b0, cnt, al && (b0 & 3) == 0, gb);
    }
}

static int pad_check(const char *what, int planes, int H, int W, int wl, int wr, int hl, int hr, PadGeom *gm, long long *in_count,
                     long long *out_count)
{
    CTPVAE_REQUIRE(planes >= 1 && H >= 1 && W >= 1, "%s: extents must be at least 1 (planes=%d H=%d W=%d)", what, planes, H, W);
    CTPVAE_REQUIRE(wl >= 0 && wr >= 0 && hl >= 0 && hr >= 0, "%s: pads must not be negative (wl=%d wr=%d hl=%d hr=%d)", what, wl, wr, hl, hr);
    const long long OH = (long long)H + hl + hr, OW = (long long)W + wl + wr;
    CTPVAE_REQUIRE(OH <= INT_MAX && OW <= INT_MAX && OH * OW <= INT_MAX && (long long)planes * (OH * OW) <= INT_MAX,
                   "%s: planes * (H + hl + hr) * (W + wl + wr) must fit 31 bits (planes=%d, %lld x %lld)", what, planes, OH, OW);
    *gm = PadGeom{H, W, (int)OH, (int)OW, (H - hl % H) % H, (W - wl % W) % W, hl % H, wl % W};
    *in_count = (long long)planes * H * W;
    *out_count = (long long)planes * OH * OW;
    return CTPVAE_OK;
}

static int maxout_check(const char *what, int n, int len)
{
    CTPVAE_REQUIRE(n >= 1 && len >= 1, "%s: extents must be at least 1 (n=%d len=%d)", what, n, len);
    CTPVAE_REQUIRE((long long)n * len <= INT_MAX / 2, "%s: 2 * n * len must fit 31 bits (n=%d len=%d)", what, n, len);
    return CTPVAE_OK;
}

static unsigned convblock_grid(unsigned quads)
{
    const unsigned blocks = (quads + kConvBlockThreads - 1) / kConvBlockThreads;
    return blocks < kConvBlockMaxGrid ? blocks : kConvBlockMaxGrid;
}

static bool convblock_aligned(const void *a, const void *b, const void *c = nullptr)
{
    return (((size_t)a | (size_t)b) & 15) == 0 && ((size_t)c & 3) == 0;   // (the byte mask is moved four bytes at a time)
}

}  // namespace ctpvae

using namespace ctpvae;

extern "C" {

int ctpvae_periodic_pad_fwd_f32(const float *x_dev, int planes, int H, int W, int wl, int wr, int hl, int hr, float *out_dev,
                                ctpvae_stream_t stream)
{
    CTPVAE_REQUIRE(x_dev && out_dev, "periodic_pad_fwd: null pointer");
    PadGeom gm;
    long long in_count, out_count;
    if (int rc = pad_check("periodic_pad_fwd", planes, H, W, wl, wr, hl, hr, &gm, &in_count, &out_count)) return rc;
    const unsigned total = (unsigned)out_count;
    hipLaunchKernelGGL(periodic_pad_fwd_kernel, dim3(convblock_grid((total + 3) / 4)), dim3(kConvBlockThreads), 0, (hipStream_t)stream, x_dev,
                       out_dev, gm, total, convblock_aligned(x_dev, out_dev) ? 1 : 0);
    CTPVAE_LAUNCH_CHECK("periodic_pad_fwd_kernel");
    return CTPVAE_OK;
}

int ctpvae_periodic_pad_bwd_f32(const float *g_dev, int planes, int H, int W, int wl, int wr, int hl, int hr, float *gx_out_dev,
                                ctpvae_stream_t stream)
{
    CTPVAE_REQUIRE(g_dev && gx_out_dev, "periodic_pad_bwd: null pointer");
    PadGeom gm;
    long long in_count, out_count;
    if (int rc = pad_check("periodic_pad_bwd", planes, H, W, wl, wr, hl, hr, &gm, &in_count, &out_count)) return rc;
    const unsigned total = (unsigned)in_count;
    hipLaunchKernelGGL(periodic_pad_bwd_kernel, dim3(convblock_grid((total + 3) / 4)), dim3(kConvBlockThreads), 0, (hipStream_t)stream, g_dev,
                       gx_out_dev, gm, total, convblock_aligned(g_dev, gx_out_dev) ? 1 : 0);
    CTPVAE_LAUNCH_CHECK("periodic_pad_bwd_kernel");
    return CTPVAE_OK;
}

int ctpvae_maxout_fwd_f32(const float *y_dev, int n, int len, float *out_dev, unsigned char *first_out_dev, ctpvae_stream_t stream)
{
    CTPVAE_REQUIRE(y_dev && out_dev && first_out_dev, "maxout_fwd: null pointer");
    if (int rc = maxout_check("maxout_fwd", n, len)) return rc;
    const unsigned qpo = ((unsigned)len + 3) / 4, quads = (unsigned)n * qpo;
    hipLaunchKernelGGL(maxout_fwd_kernel, dim3(convblock_grid(quads)), dim3(kConvBlockThreads), 0, (hipStream_t)stream, y_dev, len, qpo, quads,
                       convblock_aligned(y_dev, out_dev, first_out_dev) ? 1 : 0, out_dev, first_out_dev);
    CTPVAE_LAUNCH_CHECK("maxout_fwd_kernel");
    return CTPVAE_OK;
}

int ctpvae_maxout_bwd_f32(const float *g_dev, const unsigned char *first_dev, int n, int len, float *gy_out_dev, ctpvae_stream_t stream)
{
    CTPVAE_REQUIRE(g_dev && first_dev && gy_out_dev, "maxout_bwd: null pointer");
    if (int rc = maxout_check("maxout_bwd", n, len)) return rc;
    const unsigned qpo = ((unsigned)len + 3) / 4, quads = (unsigned)n * qpo;
    hipLaunchKernelGGL(maxout_bwd_kernel, dim3(convblock_grid(quads)), dim3(kConvBlockThreads), 0, (hipStream_t)stream, g_dev, first_dev, len,
                       qpo, quads, convblock_aligned(g_dev, gy_out_dev, first_dev) ? 1 : 0, gy_out_dev);
    CTPVAE_LAUNCH_CHECK("maxout_bwd_kernel");
    return CTPVAE_OK;
}

}  // extern "C"
