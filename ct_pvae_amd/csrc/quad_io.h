// quad_io.h -- what the four sampling operators (head.hip, beta_head.hip, latent.hip, beta_latent.hip) share around their pixel and
// element functions: positive_range, the counter words of a launch, a quad of four consecutive fp32 elements moved with one 16-byte
// access when it is whole and 16-byte aligned (guarded 4-byte accesses otherwise), a word of a Philox block picked without indexing the
// array by a run-time value, the fixed-order per-object sum of a 1024-thread workgroup, the heads' forward and backward walks, the
// latents' rows, KL walk and backward prologue, and the launch arithmetic and checks of the host side.
//
// Layout and the order of a per-object sum (head_fwd_body: LP[o] over the pixels of object o; latent_kl_walk: KL[b] over the
// elements of object b).  One workgroup of 1024 threads = 16 waves per object; no atomics.  With v_i the object's i-th term:
//   quad q of the object = its terms 4q .. 4q+3:  s_q = ((v_4q + v_4q+1) + v_4q+2) + v_4q+3              (terms past the end add +0.0f)
//   thread t takes the quads t, t + 1024, t + 2048, ...:  acc_t = ((0 + s_t) + s_(t+1024)) + ...      (a thread without a quad: +0.0f)
//   wave w = threads 64w .. 64w+63:  W_w = wave_sum(acc) -- the xor butterfly 32, 16, 8, 4, 2, 1 of loglik_math.h
//   sum = ((W_0 + W_1) + W_2) + ... + W_15                                                            (ascending, one at a time)
// The order is fixed by the term's index INSIDE its object, so the sum has the same bits whatever the number of objects, first_object
// and the object's alignment in memory are.  The longest chain of additions is 3 + ceil(ceil(terms / 4) / 1024) + 6 + 15.
// A quad of an array is moved with one 16-byte access when it is whole and 16-byte aligned in memory (every pointer of the launch
// 16-byte aligned and the row's offset a multiple of 4), with guarded 4-byte accesses otherwise.  The backwards have no sum: 256 threads
// per workgroup, one quad per thread.
#pragma once
#include <climits>
#include <initializer_list>

#include "common.h"
#include "loglik_math.h"
#include "philox.h"

namespace ctpvae {

constexpr int kObjectSumThreads = 1024;   // 16 waves per object
constexpr int kQuadBwdThreads = 256;      // the backwards: one quad per thread
constexpr float kPositiveRangeEps = 1.1920928955078125e-07f;    // FLT_EPSILON, positive_range's offset

// pr(t) = t >= 1 ? t : exp(t - 1) + EPS and its slope pr'(t) = t >= 1 ? 1 : exp(t - 1): the ONE copy (-ffp-contract=off makes the
// bits of these operations part of every operator's contract)
__device__ __forceinline__ float positive_range(float t, float &slope)
{
    const float e = expf(t - 1.0f);
    slope = t >= 1.0f ? 1.0f : e;
    return t >= 1.0f ? t : e + kPositiveRangeEps;
}

// the counter words of a launch: the 64-bit flat index of its first element (first_object * extent, extent = the elements of one
// object), the draw and the key.  An operator extends it with what else its generator takes.
struct QuadRng {
    unsigned long long first;
    unsigned draw, k0, k1;
};

inline QuadRng quad_rng(long long first_object, int extent, unsigned long long seed, unsigned draw)
{
    return QuadRng{(unsigned long long)first_object * (unsigned long long)extent, draw, (unsigned)seed, (unsigned)(seed >> 32)};
}

// word k (0 .. 3) of a block, without indexing the array by a run-time value
__host__ __device__ inline unsigned philox_word(const Philox4 &b, unsigned k)
{
    return k == 0 ? b.w[0] : (k == 1 ? b.w[1] : (k == 2 ? b.w[2] : b.w[3]));
}

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, const float (&v)[4]) { *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]); }
// the elements i .. i+cnt-1 of an array; the rest of the quad reads `fill`
__device__ __forceinline__ void quad_load(const float *p, size_t i, int cnt, bool vec, float fill, float (&v)[4])
{
    if (vec && cnt == 4) {
        const float4 q = ld4(p + i);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < cnt ? p[i + j] : fill;
    }
}
__device__ __forceinline__ void quad_store(float *p, size_t i, int cnt, bool vec, const float (&v)[4])
{
    if (vec && cnt == 4) {
        st4(p + i, v);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < cnt) p[i + j] = v[j];
    }
}

// The end of the per-object sum: acc is thread t's own partial (its quads, ascending); W_w = wave_sum(acc) of wave w (the xor
// butterfly 32, 16, 8, 4, 2, 1), then ((W_0 + W_1) + W_2) + ... + W_15 one at a time.  Every thread of the 1024 calls it; the result
// is valid in thread 0.  wsum: 16 floats of LDS.
__device__ __forceinline__ float object_sum_1024(float acc, float *wsum, int t)
{
    const float w = wave_sum(acc);
    if ((t & 63) == 0) wsum[t >> 6] = w;
    __syncthreads();
    float s = 0.0f;
    if (t == 0) {
        s = wsum[0];
#pragma unroll
        for (int k = 1; k < kObjectSumThreads / 64; ++k) s += wsum[k];
    }
    return s;
}

// ---- the heads: alpha, beta [n][pix] -------------------------------------------------------------------------------------------------
// The forward of one object (workgroup o of 1024 threads).  quad(al, be, i, cnt, vec, x, lp) evaluates the four pixels i .. i+3 (i the
// flat index of the first in the launch's arrays; those past cnt hold the fill 1.0f and their lp is not used).
template <class Quad>
__device__ __forceinline__ void head_fwd_body(const float *__restrict__ alpha, const float *__restrict__ beta, int pix, int ptr_aligned,
                                              float *__restrict__ x_out, float *__restrict__ lp_sum, float *__restrict__ lp_elem,
                                              const Quad &quad)
{
    __shared__ float wsum[kObjectSumThreads / 64];
    const int o = blockIdx.x, t = threadIdx.x;
    const size_t base = (size_t)o * pix;
    const bool vec = ptr_aligned != 0 && (base & 3) == 0;
    const int quads = (pix + 3) >> 2;
    float acc = 0.0f;
    for (int q = t; q < quads; q += kObjectSumThreads) {
        const int r = 4 * q;
        const int cnt = pix - r < 4 ? pix - r : 4;
        const size_t i = base + r;
        float al[4], be[4], x[4], lp[4];
        quad_load(alpha, i, cnt, vec, 1.0f, al);
        quad_load(beta, i, cnt, vec, 1.0f, be);
        quad(al, be, i, cnt, vec, x, lp);
#pragma unroll
        for (int j = 0; j < 4; ++j) lp[j] = j < cnt ? lp[j] : 0.0f;
        quad_store(x_out, i, cnt, vec, x);
        if (lp_elem != nullptr) quad_store(lp_elem, i, cnt, vec, lp);
        acc += ((lp[0] + lp[1]) + lp[2]) + lp[3];
    }
    const float s = object_sum_1024(acc, wsum, t);
    if (t == 0) lp_sum[o] = s;
}

// The backward: the total = n * pix pixels as memory quads, one per thread.  grad(al, be, i, cnt, vec, gx, G, ga, gb) gives the four
// pixels' (g_alpha, g_beta) for their cotangents gx (of x; zero without g_x) and G (of the pixel's object's LP; zero without g_lp).
template <class Grad>
__device__ __forceinline__ void head_bwd_body(const float *__restrict__ alpha, const float *__restrict__ beta, long long total, int pix,
                                              int ptr_aligned, const float *__restrict__ g_x, const float *__restrict__ g_lp,
                                              float *__restrict__ g_alpha, float *__restrict__ g_beta, const Grad &grad)
{
    const long long i0 = 4 * ((long long)blockIdx.x * kQuadBwdThreads + threadIdx.x);
    if (i0 >= total) return;
    const int cnt = total - i0 < 4 ? (int)(total - i0) : 4;
    const size_t i = (size_t)i0;
    const bool vec = ptr_aligned != 0;
    float al[4], be[4], gx[4], G[4], ga[4], gb[4];
    quad_load(alpha, i, cnt, vec, 1.0f, al);
    quad_load(beta, i, cnt, vec, 1.0f, be);
    if (g_x != nullptr) quad_load(g_x, i, cnt, vec, 0.0f, gx);
    else gx[0] = gx[1] = gx[2] = gx[3] = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // the pixel's object: total < 2^31, so 32-bit division (pixels past the end read object n - 1 and are not stored)
        const unsigned e = (unsigned)(j < cnt ? i0 + j : i0);
        G[j] = g_lp != nullptr ? g_lp[e / (unsigned)pix] : 0.0f;
    }
    grad(al, be, i, cnt, vec, gx, G, ga, gb);
    quad_store(g_alpha, i, cnt, vec, ga);
    quad_store(g_beta, i, cnt, vec, gb);
}

// ---- the latents: skip [B][2C][H][W], len = C H W; object b's loc row at 2 b len, its log_scale row at 2 b len + len ------------------
__host__ __device__ inline int quad_count(int len) { return (len >> 2) + ((len & 3) != 0); }

// the offsets of object b's rows -- loc and log_scale in skip (and g_skip), el in a [B][len] array -- and whether their quads may move
// 16 bytes at a time; `al`: every pointer of the launch is 16-byte aligned
struct LatentRows {
    size_t loc0, ls0, el0;
    bool al, vec_loc, vec_ls, vec_el;
};

__device__ __forceinline__ LatentRows latent_rows(int b, int len, int ptr_aligned)
{
    LatentRows w;
    const size_t L = (size_t)len;
    w.loc0 = 2 * (size_t)b * L, w.ls0 = w.loc0 + L, w.el0 = (size_t)b * L;
    w.al = ptr_aligned != 0;
    w.vec_loc = w.al && (w.loc0 & 3) == 0, w.vec_ls = w.al && (w.ls0 & 3) == 0, w.vec_el = w.al && (w.el0 & 3) == 0;
    return w;
}

// The KL of object b (a workgroup of 1024 threads).  kl_of(w, r, cnt, loc, ls, kl) gives the KL terms of the elements r .. r+3 of the
// object from their loc and log_scale (those past cnt hold loc_fill and 1.0f, and their kl is not used); it may do the quad's other
// work in the same pass.  kl_sum may be null.
template <class Kl>
__device__ __forceinline__ void latent_kl_walk(const float *__restrict__ skip, int b, int len, int ptr_aligned, float loc_fill,
                                               float *__restrict__ kl_sum, float *__restrict__ kl_elem, const Kl &kl_of)
{
    __shared__ float wsum[kObjectSumThreads / 64];
    const int t = threadIdx.x;
    const LatentRows w = latent_rows(b, len, ptr_aligned);
    const int quads = quad_count(len);
    float acc = 0.0f;
    for (int q = t; q < quads; q += kObjectSumThreads) {
        const int r = 4 * q;
        const int cnt = len - r < 4 ? len - r : 4;
        float loc[4], ls[4], kl[4];
        quad_load(skip, w.loc0 + r, cnt, w.vec_loc, loc_fill, loc);
        quad_load(skip, w.ls0 + r, cnt, w.vec_ls, 1.0f, ls);
        kl_of(w, r, cnt, loc, ls, kl);
#pragma unroll
        for (int j = 0; j < 4; ++j) kl[j] = j < cnt ? kl[j] : 0.0f;
        if (kl_elem != nullptr) quad_store(kl_elem, w.el0 + r, cnt, w.vec_el, kl);
        acc += ((kl[0] + kl[1]) + kl[2]) + kl[3];
    }
    const float total = object_sum_1024(acc, wsum, t);
    if (t == 0 && kl_sum != nullptr) kl_sum[b] = total;
}

// The backward's quad: workgroup blockIdx.x of 256 threads is one of object b's blocks_per_object; false: the thread has no quad.
__device__ __forceinline__ bool latent_bwd_quad(int len, int blocks_per_object, int &b, int &r, int &cnt)
{
    b = blockIdx.x / blocks_per_object;
    const int q = (blockIdx.x - b * blocks_per_object) * kQuadBwdThreads + threadIdx.x;
    r = 4 * q;
    cnt = len - r < 4 ? len - r : 4;
    return q < quad_count(len);
}

// ---- the host side -------------------------------------------------------------------------------------------------------------------
inline bool head_aligned16(std::initializer_list<const void *> ptrs)
{
    for (const void *p : ptrs)
        if (((size_t)p & 15) != 0) return false;   // (a null pointer counts as aligned)
    return true;
}

// workgroups of a head's backward: total = n * pix < 2^31 pixels
inline unsigned head_bwd_grid(long long total) { return (unsigned)((total + 4ll * kQuadBwdThreads - 1) / (4ll * kQuadBwdThreads)); }
// workgroups per object of a latent backward: B * blocks <= B * len < 2^31
inline int latent_blocks_per_object(int len) { return (quad_count(len) + kQuadBwdThreads - 1) / kQuadBwdThreads; }

inline int head_size_check(const char *what, int n, int pix, long long first_object)
{
    CTPVAE_REQUIRE(n > 0 && pix > 0, "%s: sizes must be positive (n=%d pix=%d)", what, n, pix);
    CTPVAE_REQUIRE((long long)n * pix <= INT_MAX, "%s: n * pix must fit 31 bits (n=%d pix=%d)", what, n, pix);
    CTPVAE_REQUIRE(first_object >= 0 && first_object <= LLONG_MAX / pix - n,
                   "%s: first_object must be >= 0 and (first_object + n) * pix must fit 63 bits (got %lld)", what, first_object);
    return CTPVAE_OK;
}

inline int head_check(const char *what, const void *alpha, const void *beta, int n, int pix, long long first_object)
{
    CTPVAE_REQUIRE(alpha && beta, "%s: null pointer", what);
    return head_size_check(what, n, pix, first_object);
}

// max_ns: what the operator's fourth counter word leaves for the sample index
inline int latent_check(const char *what, int B, int len, int ns, int max_ns, long long first_object, unsigned level)
{
    CTPVAE_REQUIRE(B > 0 && len > 0 && ns > 0, "%s: sizes must be positive (B=%d len=%d ns=%d)", what, B, len, ns);
    CTPVAE_REQUIRE(ns <= max_ns, "%s: ns must be at most %d (got %d)", what, max_ns, ns);
    CTPVAE_REQUIRE(level <= 255u, "%s: level must be at most 255 (got %u)", what, level);
    CTPVAE_REQUIRE((long long)ns * B <= INT_MAX && (long long)ns * B * len <= INT_MAX,
                   "%s: ns * B * len must fit 31 bits (B=%d len=%d ns=%d)", what, B, len, ns);
    CTPVAE_REQUIRE(first_object >= 0 && first_object <= LLONG_MAX / len - B,
                   "%s: first_object must be >= 0 and (first_object + B) * len must fit 63 bits (got %lld)", what, first_object);
    return CTPVAE_OK;
}

}  // namespace ctpvae
