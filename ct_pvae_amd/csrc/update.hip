// update.hip -- the update stage of a P-VAE training step (ctvae/main_ct_vae.py:353, :482-485: tf.where(is_nan, 0, g), tf.clip_by_norm(g,
// norm) per tensor, tf.keras.optimizers.Adam(lr, epsilon).apply_gradients) as TWO launches over the flat gradient buffer of
// sharding.FlatGradBucket, whatever the number of tensors: no atomics, no step counter on the device, nothing read back.
//
// Operands.  grad [total] float32, read only: the reduced gradients of T tensors back to back, tensor k at the element offset
// len_0 + .. + len_(k-1) -- any offset, no padding.  m, v [total] float32: Adam's two moments, resident, in the same layout.  The
// parameters are not flat: they stay the tensors their modules own, and the chunk table carries their addresses.
//
// The chunk table (host-built, ctpvae_update_plan_host; C = kUpdateChunk = 1024 elements): tensor k is cut into ceil(len_k / C)
// chunks, all of C elements but the last; the chunks of tensor 0 come first, ascending in offset, then those of tensor 1, ... -- so no
// chunk crosses a tensor boundary, none is longer than C, and the table ascends in offset.  One 32-byte record per chunk: its flat
// offset, the address of the parameter's element that belongs to the chunk's first, its length, its tensor, the index of its tensor's
// first chunk and the number of chunks of its tensor.  One workgroup of 256 threads takes one chunk in both launches; thread t owns the
// chunk's elements 4t .. 4t+3 (the quad t of the CHUNK, not of memory: the order below does not depend on where a tensor starts).
//
// Launch 1, the norms.  g0 = isnan(g) ? 0 : g;  d_i = (double)g0_i * (double)g0_i (exact: 48 bits of product in 53).  Per chunk, in float64:
//   s_t   = ((d_4t + d_4t+1) + d_4t+2) + d_4t+3                       (elements past the chunk's end add +0.0)
//   W_w   = the xor butterfly 32, 16, 8, 4, 2, 1 over the 64 lanes of wave w:  x_l <- x_l + x_(l ^ 32), then ^ 16, ... (every lane ends
//           with the same bits: each level adds the same two numbers in both lanes of a pair)
//   part  = ((W_0 + W_1) + W_2) + W_3                                  -> partials[chunk], one float64 per chunk
// Launch 2, the update.  Every workgroup first adds the partials of ITS tensor, one at a time in ascending chunk order, in float64:
//   sum = ((0 + part_first) + part_(first+1)) + ...;   l2 = (float)sqrt(sum)     (IEEE sqrt, one rounding to float32)
// (every workgroup of a tensor repeats that sum -- count dependent additions each; 64 partials are fetched at a time through LDS.  The
// c3 model's largest tensor, 84480 elements, has 83 chunks.)  The workgroup of a tensor's first chunk stores l2 into norms[tensor].  Then per
// element, float32, each line one correctly rounded operation after the other (the library is built with -ffp-contract=off):
//   g0 = isnan(g) ? 0 : g
//   gc = (g0 * clip) / fmaxf(l2, clip)            tf.clip_by_norm's own form: no branch, an unclipped tensor is (g * clip) / clip, not g
//   m += (gc - m) * (1.0f - b1)
//   v += (gc * gc - v) * (1.0f - b2)
//   p -= (m * alpha) / (sqrtf(v) + eps)
// [3P-recalled] the last three lines are TensorFlow's ApplyAdam functor (tensorflow/core/kernels/training_ops.cc, non-Nesterov), the
// second tf.clip_by_norm (python/ops/clip_ops.py: values * clip_norm / maximum(l2norm, clip_norm)), both written down from memory: the
// reference ships no TensorFlow source.  Epsilon stands OUTSIDE the bias correction ("epsilon hat"), where torch.optim.Adam puts it
// inside.  Two stated deviations from TensorFlow: alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t) comes from the host, evaluated in
// float64 and rounded once (TensorFlow evaluates it in float32); and the squared norm is summed in float64 in the order above
// (TensorFlow's reduce_sum is float32, its order unspecified).  An inf in a tensor makes l2 = inf: its finite elements give gc = 0, the
// inf itself NaN, as the formula says.
//
// Memory: a quad is moved with one 16-byte access when it is whole and 16-byte aligned in memory -- for grad, m and v: the three base
// pointers aligned and the tensor's flat offset a multiple of 4; for the parameter: its own address -- and with guarded 4-byte accesses
// otherwise.  The values do not depend on which.  Bandwidth-bound: 7 float32 streams of `total` elements in launch 2, 1 in launch 1.
#include <climits>
#include <cmath>

#include "common.h"
#include "quad_io.h"

namespace ctpvae {

constexpr int kUpdateChunk = 1024;
constexpr int kUpdateThreads = kUpdateChunk / 4;
constexpr int kUpdateStage = 64;           // partials fetched per round of launch 2's sum

struct UpdateChunk {
    long long off;      // flat element offset of the chunk's first element
    float *param;       // the parameter's element at that offset
    int len;            // 1 .. kUpdateChunk
    int tensor;
    int first;          // index of the tensor's first chunk
    int count;          // chunks of the tensor
};
static_assert(sizeof(UpdateChunk) == 32, "the chunk table's record is 32 bytes");

struct UpdateScalars {
    float alpha, clip, b1, b2, eps;
};

__device__ __forceinline__ double update_wave_sum(double x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = x + __shfl_xor(x, off, 64);
    return x;
}

__global__ __launch_bounds__(kUpdateThreads) void update_norm_kernel(const UpdateChunk *__restrict__ plan, const float *__restrict__ grad,
                                                                      int flat_aligned, double *__restrict__ partials)
{
    __shared__ double wsum[kUpdateThreads / 64];
    const UpdateChunk c = plan[blockIdx.x];
    const int t = threadIdx.x, r = 4 * t;
    const int cnt = c.len - r < 4 ? (c.len - r > 0 ? c.len - r : 0) : 4;
    float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (cnt > 0) quad_load(grad, (size_t)c.off + r, cnt, flat_aligned != 0 && (c.off & 3) == 0, 0.0f, g);
    double d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double g0 = isnan(g[j]) ? 0.0 : (double)g[j];
        d[j] = g0 * g0;
    }
    const double w = update_wave_sum(((d[0] + d[1]) + d[2]) + d[3]);
    if ((t & 63) == 0) wsum[t >> 6] = w;
    __syncthreads();
    if (t == 0) partials[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ __launch_bounds__(kUpdateThreads) void update_apply_kernel(const UpdateChunk *__restrict__ plan, const float *__restrict__ grad,
                                                                       float *__restrict__ m, float *__restrict__ v,
                                                                       const double *__restrict__ partials, int flat_aligned, UpdateScalars s,
                                                                       float *__restrict__ norms)
{
    __shared__ double stage[kUpdateStage];
    const UpdateChunk c = plan[blockIdx.x];
    const int t = threadIdx.x;
    double sum = 0.0;
    for (int k0 = 0; k0 < c.count; k0 += kUpdateStage) {
        const int n = c.count - k0 < kUpdateStage ? c.count - k0 : kUpdateStage;
        if (t < n) stage[t] = partials[c.first + k0 + t];
        __syncthreads();
        for (int i = 0; i < n; ++i) sum += stage[i];
        __syncthreads();
    }
    const float l2 = (float)sqrt(sum);
    if (t == 0 && (int)blockIdx.x == c.first) norms[c.tensor] = l2;
    const int r = 4 * t;
    if (r >= c.len) return;
    const int cnt = c.len - r < 4 ? c.len - r : 4;
    const bool vec_flat = flat_aligned != 0 && (c.off & 3) == 0, vec_p = ((size_t)c.param & 15) == 0;
    const size_t i = (size_t)c.off + r;
    float g[4], mm[4], vv[4], p[4];
    quad_load(grad, i, cnt, vec_flat, 0.0f, g);
    quad_load(m, i, cnt, vec_flat, 0.0f, mm);
    quad_load(v, i, cnt, vec_flat, 0.0f, vv);
    quad_load(c.param, (size_t)r, cnt, vec_p, 0.0f, p);
    const float denom = fmaxf(l2, s.clip), omb1 = 1.0f - s.b1, omb2 = 1.0f - s.b2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float g0 = isnan(g[j]) ? 0.0f : g[j];
        const float gc = (g0 * s.clip) / denom;
        mm[j] += (gc - mm[j]) * omb1;
        vv[j] += (gc * gc - vv[j]) * omb2;
        p[j] -= (mm[j] * s.alpha) / (sqrtf(vv[j]) + s.eps);
    }
    quad_store(m, i, cnt, vec_flat, mm);
    quad_store(v, i, cnt, vec_flat, vv);
    quad_store(c.param, (size_t)r, cnt, vec_p, p);
}

// the number of chunks of T tensors, or a negative code
static long long update_count_chunks(const char *what, const long long *lens_host, int T)
{
    if (lens_host == nullptr) return fail(CTPVAE_EINVAL, "%s: null pointer", what);
    if (T <= 0) return fail(CTPVAE_EINVAL, "%s: the tensor list is empty (T=%d)", what, T);
    long long chunks = 0, total = 0;
    for (int k = 0; k < T; ++k) {
        const long long len = lens_host[k];
        if (len <= 0) return fail(CTPVAE_EINVAL, "%s: tensor %d has length %lld: every length must be positive", what, k, len);
        if (len > LLONG_MAX / 8 - total) return fail(CTPVAE_EINVAL, "%s: the lengths do not add up in 60 bits", what);
        total += len;
        chunks += (len + kUpdateChunk - 1) / kUpdateChunk;
    }
    if (chunks > INT_MAX) return fail(CTPVAE_EINVAL, "%s: %lld chunks, more than a launch has workgroups (2^31 - 1)", what, chunks);
    return chunks;
}

}  // namespace ctpvae

using namespace ctpvae;

extern "C" {

int ctpvae_update_chunk_len(void) { return kUpdateChunk; }

long long ctpvae_update_plan_bytes(const long long *lens_host, int T)
{
    const long long chunks = update_count_chunks("update_plan_bytes", lens_host, T);
    return chunks < 0 ? chunks : chunks * (long long)sizeof(UpdateChunk);
}

int ctpvae_update_plan_host(const long long *lens_host, const void *const *params_host, int T, void *plan_out_host)
{
    CTPVAE_REQUIRE(lens_host && params_host && plan_out_host, "update_plan_host: null pointer");
    const long long chunks = update_count_chunks("update_plan_host", lens_host, T);
    if (chunks < 0) return (int)chunks;
    for (int k = 0; k < T; ++k) {
        CTPVAE_REQUIRE(params_host[k] != nullptr, "update_plan_host: parameter %d has a null address", k);
        CTPVAE_REQUIRE(((size_t)params_host[k] & 3) == 0, "update_plan_host: parameter %d is not 4-byte aligned", k);
    }
    UpdateChunk *out = static_cast<UpdateChunk *>(plan_out_host);
    long long off = 0;
    int c = 0;
    for (int k = 0; k < T; ++k) {
        const long long len = lens_host[k];
        const int count = (int)((len + kUpdateChunk - 1) / kUpdateChunk), first = c;
        for (int j = 0; j < count; ++j, ++c) {
            const long long at = (long long)j * kUpdateChunk;
            out[c].off = off + at;
            out[c].param = static_cast<float *>(const_cast<void *>(params_host[k])) + at;
            out[c].len = (int)(len - at < kUpdateChunk ? len - at : kUpdateChunk);
            out[c].tensor = k;
            out[c].first = first;
            out[c].count = count;
        }
        off += len;
    }
    return CTPVAE_OK;
}

int ctpvae_update_f32(const void *plan_dev, int n_chunks, int T, const float *grad_dev, float *m_dev, float *v_dev, double *partials_dev,
                      float *norms_out_dev, long long t, float alpha, float clip, float b1, float b2, float eps, ctpvae_stream_t stream)
{
    CTPVAE_REQUIRE(plan_dev && grad_dev && m_dev && v_dev && partials_dev && norms_out_dev, "update: null pointer");
    CTPVAE_REQUIRE(T > 0 && n_chunks >= T, "update: needs T >= 1 tensors and at least one chunk each (T=%d n_chunks=%d)", T, n_chunks);
    CTPVAE_REQUIRE(((size_t)plan_dev & 7) == 0 && ((size_t)partials_dev & 7) == 0, "update: the chunk table and the partials must be 8-byte aligned");
    CTPVAE_REQUIRE((((size_t)grad_dev | (size_t)m_dev | (size_t)v_dev | (size_t)norms_out_dev) & 3) == 0, "update: a float32 buffer is not 4-byte aligned");
    CTPVAE_REQUIRE(t >= 1, "update: the step count t starts at 1 (got %lld)", t);
    CTPVAE_REQUIRE(std::isfinite(alpha) && clip > 0.0f && std::isfinite(clip), "update: alpha must be finite and clip positive and finite "
                   "(alpha=%g clip=%g)", (double)alpha, (double)clip);
    CTPVAE_REQUIRE(b1 >= 0.0f && b1 < 1.0f && b2 >= 0.0f && b2 < 1.0f && eps >= 0.0f && std::isfinite(eps),
                   "update: needs 0 <= b1, b2 < 1 and a finite eps >= 0 (b1=%g b2=%g eps=%g)", (double)b1, (double)b2, (double)eps);
    const int aligned = ((((size_t)grad_dev | (size_t)m_dev | (size_t)v_dev) & 15) == 0) ? 1 : 0;
    const UpdateChunk *plan = static_cast<const UpdateChunk *>(plan_dev);
    hipLaunchKernelGGL(update_norm_kernel, dim3((unsigned)n_chunks), dim3(kUpdateThreads), 0, (hipStream_t)stream, plan, grad_dev, aligned,
                       partials_dev);
    CTPVAE_LAUNCH_CHECK("update_norm_kernel");
    hipLaunchKernelGGL(update_apply_kernel, dim3((unsigned)n_chunks), dim3(kUpdateThreads), 0, (hipStream_t)stream, plan, grad_dev, m_dev, v_dev,
                       partials_dev, aligned, UpdateScalars{alpha, clip, b1, b2, eps}, norms_out_dev);
    CTPVAE_LAUNCH_CHECK("update_apply_kernel");
    return CTPVAE_OK;
}

}  // extern "C"
