// quad_io.h -- what the per-object kernels of head.hip and latent.hip share: a quad of four consecutive fp32 elements moved with one
// 16-byte access when it is whole and 16-byte aligned (guarded 4-byte accesses otherwise), a word of a Philox block picked without
// indexing the array by a run-time value, and the last two levels of the fixed-order per-object sum of a 1024-thread workgroup.
#pragma once
#include "loglik_math.h"
#include "philox.h"

namespace ctpvae {

constexpr int kObjectSumThreads = 1024;   // 16 waves per object

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

}  // namespace ctpvae
