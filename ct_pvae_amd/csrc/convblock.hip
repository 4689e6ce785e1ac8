// convblock.hip -- the glue around every convolution of the P-VAE's ConvBlock (ctvae/models.py:219-263, :330-341;
// ct_pvae_amd/trainer.py _PeriodicPad and _Maxout) as ONE launch each way: the 'periodic' padding of the two spatial axes and the
// maxout of the two channel halves, and the block's dropout, alone or inside the pad's launches.  All kernels are pure streaming on
// contiguous fp32 [N][C][H][W] tensors: no LDS, no atomics, no floating-point arithmetic but the backward's additions and the
// dropout's one multiply.
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
// Dropout (ctvae/models.py:58-61, :141-144, :283-284: "Dropout => Conv2D => Maxout", on the block's input before the padding), as a
// counter-based stream like head.hip's and latent.hip's: Philox4x32-10 (philox.h), key = seed.  The block input is [N][C][H][W],
// len = C * H * W; element i of object n has the 64-bit flat index e = (first_object + n) * len + i and takes word w = e & 3 of the
// block with counter (lo32(e >> 2), hi32(e >> 2), draw, 0x44000000 | layer), layer < 2^24 (the top byte 0x44 keeps the fourth counter
// word apart from latent.hip's 0x4C......, head.hip's 0x544E48, hmc.hip's 0x484D43 and poisson.hip's 0).
//   keep       (w >> 8) >= T, T = ceil(float32(rate) * 2^24) made by the host: u = (w >> 8) * 2^-24 >= float32(rate)
//   forward    out = keep ? x * scale : +0.0f, scale = float32(1 / (1 - rate)) made by the host; ONE fp32 multiply
//   backward   gx = keep ? scale * acc : +0.0f, acc the cotangent (dropout_bwd) or the two folds above, unchanged (dropout_pad_bwd)
//   a dropped element is a SELECTION, not a product with 0: a dropped inf or NaN gives +0 (TensorFlow's x * scale * mask gives NaN),
//   as the maxout's backward selects.  The backward draws the mask again from the same (seed, draw, layer, first_object): nothing
//   is kept for it.  dropout_pad_fwd keys the decision by the SOURCE element, so every wrapped copy of an element shares its fate:
//   out[p][r][q] = drop(x)[p][(r - hl) mod H][(q - wl) mod W], the bits of periodic_pad(dropout(x)).
//   One Philox block serves four consecutive flat indices: a quad whose four sources are consecutive computes one block when its
//   first e is a multiple of 4 and two when it is not (first_object * len is no multiple of 4, or an unaligned padded row); a quad
//   whose sources wrap computes a block only where the block index changes from one source to the next.
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

constexpr unsigned kDropTag = 0x44000000u;   // 'D' in the top byte of the fourth counter word; the layer below

struct DropKey {
    unsigned long long e0;   // first_object * len: the flat index of the call's first element
    unsigned draw, tag;      // tag = kDropTag | layer
    unsigned k0, k1;         // the seed's two halves
    unsigned T;              // keep iff (w >> 8) >= T
    float scale;
};

__host__ __device__ inline Philox4 drop_block(const DropKey &key, unsigned long long blk)
{
    return philox4x32_10((unsigned)blk, (unsigned)(blk >> 32), key.draw, key.tag, key.k0, key.k1);
}

// the keep decision of one element, with the block of the element before it: a new block only where the block index changes
struct DropCursor {
    unsigned long long blk;
    Philox4 b;
    bool have;
};
__host__ __device__ inline bool drop_keep(const DropKey &key, DropCursor &c, unsigned long long e)
{
    const unsigned long long blk = e >> 2;
    if (!c.have || blk != c.blk) c.b = drop_block(key, blk), c.blk = blk, c.have = true;
    return (philox_word(c.b, (unsigned)e & 3u) >> 8) >= key.T;
}

// bit k: element e + k is kept, k < cnt <= 4 -- one block when e is a multiple of 4, two when the quad straddles
__host__ __device__ inline unsigned drop_keep4(const DropKey &key, unsigned long long e, int cnt)
{
    const unsigned s = (unsigned)e & 3u;
    const Philox4 a = drop_block(key, e >> 2);
    unsigned bits = 0;
    if (s == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) bits |= ((a.w[k] >> 8) >= key.T ? 1u : 0u) << k;
    } else {
        Philox4 b = a;
        if (s + (unsigned)cnt > 4u) b = drop_block(key, (e >> 2) + 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned i = s + (unsigned)k;
            const unsigned w = i < 4u ? philox_word(a, i) : philox_word(b, i - 4u);
            bits |= ((w >> 8) >= key.T ? 1u : 0u) << k;
        }
    }
    return bits;
}

__device__ __forceinline__ void drop_apply4(const DropKey &key, unsigned bits, float (&v)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = ((bits >> k) & 1u) != 0 ? v[k] * key.scale : 0.0f;
}

// out quad e .. e+3 of the flat padded array [planes][OH][OW]; kDrop: the source elements dropped (keyed by their own flat index)
template <bool kDrop>
__global__ __launch_bounds__(kConvBlockThreads) void periodic_pad_fwd_kernel(const float *__restrict__ x, float *__restrict__ out, PadGeom gm,
                                                                              unsigned total, int ptr_aligned, DropKey key)
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
            if constexpr (kDrop) drop_apply4(key, drop_keep4(key, key.e0 + (src + sq), 4), v);     // a source quad: one block
        } else {
            [[maybe_unused]] DropCursor cur{0, {}, false};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = j < cnt ? x[src + sq] : 0.0f;
                if constexpr (kDrop)
                    if (j < cnt) v[j] = drop_keep(key, cur, key.e0 + (src + sq)) ? v[j] * key.scale : 0.0f;
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

// gx quad e .. e+3 of the flat source array [planes][H][W]; kDrop: masked and scaled at the source element, after the folds
template <bool kDrop>
__global__ __launch_bounds__(kConvBlockThreads) void periodic_pad_bwd_kernel(const float *__restrict__ g, float *__restrict__ gx, PadGeom gm,
                                                                              unsigned total, int ptr_aligned, DropKey key)
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
        if constexpr (kDrop) drop_apply4(key, drop_keep4(key, key.e0 + e, cnt), acc);    // the quad's sources are consecutive
        quad_store(gx, e, cnt, al, acc);
    }
}

// out quad e .. e+3 of the flat array [n][len]: the standalone dropout, and its backward with the cotangent as x (a multiply commutes)
__global__ __launch_bounds__(kConvBlockThreads) void dropout_kernel(const float *__restrict__ x, float *__restrict__ out, unsigned total,
                                                                     int ptr_aligned, DropKey key)
{
    const unsigned quads = (total >> 2) + ((total & 3u) != 0);
    const bool al = ptr_aligned != 0;
    for (unsigned qd = blockIdx.x * kConvBlockThreads + threadIdx.x; qd < quads; qd += gridDim.x * kConvBlockThreads) {
        const unsigned e = 4u * qd;
        const int cnt = total - e < 4u ? (int)(total - e) : 4;
        float v[4];
        quad_load(x, e, cnt, al, 0.0f, v);
        drop_apply4(key, drop_keep4(key, key.e0 + e, cnt), v);
        quad_store(out, e, cnt, al, v);
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

// n objects of len elements each; T and scale as the host made them from the rate
static int dropout_check(const char *what, int n, long long len, long long first_object, unsigned long long seed, unsigned draw,
                         unsigned layer, unsigned T, float scale, DropKey *key)
{
    CTPVAE_REQUIRE(n >= 1 && len >= 1, "%s: extents must be at least 1 (n=%d len=%lld)", what, n, len);
    CTPVAE_REQUIRE((long long)n * len <= INT_MAX, "%s: n * len must fit 31 bits (n=%d len=%lld)", what, n, len);
    CTPVAE_REQUIRE(layer < (1u << 24), "%s: layer must be below 2^24 (got %u)", what, layer);
    CTPVAE_REQUIRE(T >= 1u && T < (1u << 24), "%s: T = ceil(float32(rate) * 2^24) must be in 1 .. 2^24 - 1, 0 < rate < 1 (got %u)", what, T);
    CTPVAE_REQUIRE(scale >= 1.0f && scale <= 16777216.0f, "%s: scale = 1 / (1 - rate) must be in 1 .. 2^24 (got %g)", what, (double)scale);
    CTPVAE_REQUIRE(first_object >= 0 && first_object <= LLONG_MAX / len - n,
                   "%s: first_object must be >= 0 and (first_object + n) * len must fit 63 bits (got %lld)", what, first_object);
    *key = DropKey{(unsigned long long)first_object * (unsigned long long)len, draw, kDropTag | layer, (unsigned)seed, (unsigned)(seed >> 32),
                   T, scale};
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
    hipLaunchKernelGGL(periodic_pad_fwd_kernel<false>, dim3(convblock_grid((total + 3) / 4)), dim3(kConvBlockThreads), 0, (hipStream_t)stream,
                       x_dev, out_dev, gm, total, convblock_aligned(x_dev, out_dev) ? 1 : 0, DropKey{});
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
    hipLaunchKernelGGL(periodic_pad_bwd_kernel<false>, dim3(convblock_grid((total + 3) / 4)), dim3(kConvBlockThreads), 0, (hipStream_t)stream,
                       g_dev, gx_out_dev, gm, total, convblock_aligned(g_dev, gx_out_dev) ? 1 : 0, DropKey{});
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

static int dropout_launch(const char *what, const float *in_dev, int n, int len, long long first_object, unsigned long long seed, unsigned draw,
                          unsigned layer, unsigned T, float scale, float *out_dev, ctpvae_stream_t stream)
{
    CTPVAE_REQUIRE(in_dev && out_dev, "%s: null pointer", what);
    DropKey key;
    if (int rc = dropout_check(what, n, len, first_object, seed, draw, layer, T, scale, &key)) return rc;
    const unsigned total = (unsigned)n * (unsigned)len;
    hipLaunchKernelGGL(dropout_kernel, dim3(convblock_grid((total + 3) / 4)), dim3(kConvBlockThreads), 0, (hipStream_t)stream, in_dev, out_dev,
                       total, convblock_aligned(in_dev, out_dev) ? 1 : 0, key);
    CTPVAE_LAUNCH_CHECK("dropout_kernel");
    return CTPVAE_OK;
}

int ctpvae_dropout_fwd_f32(const float *x_dev, int n, int len, long long first_object, unsigned long long seed, unsigned draw, unsigned layer,
                           unsigned T, float scale, float *out_dev, ctpvae_stream_t stream)
{
    return dropout_launch("dropout_fwd", x_dev, n, len, first_object, seed, draw, layer, T, scale, out_dev, stream);
}

int ctpvae_dropout_bwd_f32(const float *g_dev, int n, int len, long long first_object, unsigned long long seed, unsigned draw, unsigned layer,
                           unsigned T, float scale, float *gx_out_dev, ctpvae_stream_t stream)
{
    return dropout_launch("dropout_bwd", g_dev, n, len, first_object, seed, draw, layer, T, scale, gx_out_dev, stream);
}

static int dropout_pad_check(const char *what, int n, int channels, int H, int W, int wl, int wr, int hl, int hr, long long first_object,
                             unsigned long long seed, unsigned draw, unsigned layer, unsigned T, float scale, PadGeom *gm, DropKey *key,
                             long long *in_count, long long *out_count)
{
    CTPVAE_REQUIRE(n >= 1 && channels >= 1 && (long long)n * channels <= INT_MAX, "%s: n and channels must be at least 1 and n * channels fit "
                   "31 bits (n=%d channels=%d)", what, n, channels);
    if (int rc = pad_check(what, n * channels, H, W, wl, wr, hl, hr, gm, in_count, out_count)) return rc;
    return dropout_check(what, n, *in_count / n, first_object, seed, draw, layer, T, scale, key);
}

int ctpvae_dropout_pad_fwd_f32(const float *x_dev, int n, int channels, int H, int W, int wl, int wr, int hl, int hr, long long first_object,
                               unsigned long long seed, unsigned draw, unsigned layer, unsigned T, float scale, float *out_dev,
                               ctpvae_stream_t stream)
{
    CTPVAE_REQUIRE(x_dev && out_dev, "dropout_pad_fwd: null pointer");
    PadGeom gm;
    DropKey key;
    long long in_count, out_count;
    if (int rc = dropout_pad_check("dropout_pad_fwd", n, channels, H, W, wl, wr, hl, hr, first_object, seed, draw, layer, T, scale, &gm, &key,
                                   &in_count, &out_count))
        return rc;
    const unsigned total = (unsigned)out_count;
    hipLaunchKernelGGL(periodic_pad_fwd_kernel<true>, dim3(convblock_grid((total + 3) / 4)), dim3(kConvBlockThreads), 0, (hipStream_t)stream,
                       x_dev, out_dev, gm, total, convblock_aligned(x_dev, out_dev) ? 1 : 0, key);
    CTPVAE_LAUNCH_CHECK("dropout_pad_fwd_kernel");
    return CTPVAE_OK;
}

int ctpvae_dropout_pad_bwd_f32(const float *g_dev, int n, int channels, int H, int W, int wl, int wr, int hl, int hr, long long first_object,
                               unsigned long long seed, unsigned draw, unsigned layer, unsigned T, float scale, float *gx_out_dev,
                               ctpvae_stream_t stream)
{
    CTPVAE_REQUIRE(g_dev && gx_out_dev, "dropout_pad_bwd: null pointer");
    PadGeom gm;
    DropKey key;
    long long in_count, out_count;
    if (int rc = dropout_pad_check("dropout_pad_bwd", n, channels, H, W, wl, wr, hl, hr, first_object, seed, draw, layer, T, scale, &gm, &key,
                                   &in_count, &out_count))
        return rc;
    const unsigned total = (unsigned)in_count;
    hipLaunchKernelGGL(periodic_pad_bwd_kernel<true>, dim3(convblock_grid((total + 3) / 4)), dim3(kConvBlockThreads), 0, (hipStream_t)stream,
                       g_dev, gx_out_dev, gm, total, convblock_aligned(g_dev, gx_out_dev) ? 1 : 0, key);
    CTPVAE_LAUNCH_CHECK("dropout_pad_bwd_kernel");
    return CTPVAE_OK;
}

// the keep decisions of n objects of len elements into HOST memory, one byte each (1 = kept): needs no GPU; n * len is not limited
int ctpvae_dropout_keep_host_u8(int n, int len, long long first_object, unsigned long long seed, unsigned draw, unsigned layer, unsigned T,
                                unsigned char *out_host)
{
    CTPVAE_REQUIRE(out_host, "dropout_keep_host: null pointer");
    CTPVAE_REQUIRE(n >= 1 && len >= 1, "dropout_keep_host: extents must be at least 1 (n=%d len=%d)", n, len);
    CTPVAE_REQUIRE(layer < (1u << 24), "dropout_keep_host: layer must be below 2^24 (got %u)", layer);
    CTPVAE_REQUIRE(T >= 1u && T < (1u << 24), "dropout_keep_host: T must be in 1 .. 2^24 - 1 (got %u)", T);
    CTPVAE_REQUIRE(first_object >= 0 && first_object <= LLONG_MAX / len - n,
                   "dropout_keep_host: first_object must be >= 0 and (first_object + n) * len must fit 63 bits (got %lld)", first_object);
    const DropKey key{(unsigned long long)first_object * (unsigned long long)len, draw, kDropTag | layer, (unsigned)seed, (unsigned)(seed >> 32),
                      T, 1.0f};
    DropCursor cur{0, {}, false};
    const long long total = (long long)n * len;
    for (long long i = 0; i < total; ++i) out_host[i] = drop_keep(key, cur, key.e0 + (unsigned long long)i) ? 1 : 0;
    return CTPVAE_OK;
}

}  // extern "C"
