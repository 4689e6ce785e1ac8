// conv.hip -- the convolution of a padded (non-transposed) ConvBlock (ctvae/models.py:219-263; ct_pvae_amd/trainer.py ConvBlock) with
// its periodic padding in front and its maxout behind, as ONE forward launch and at most four backward launches, on the matrix cores
// with fp32 operands (v_mfma_f32_32x32x2_f32).  Every sum has ONE stated order; no atomics; nothing depends on the device, its CU
// count, a knob or launch-time state; tests/np_twin_conv.py restates this header and the kernels are held to it BY BITS.
//
// Operands, all contiguous fp32 NCHW: x [N][Cin][H][W], w [2C][Cin][k][k] (ConvBlock.ab.weight), b [2C], stride s, pads
// (wl, wr, hl, hr) >= 0.  PH = H + hl + hr, PW = W + wl + wr, OH = (PH - k) / s + 1, OW = (PW - k) / s + 1, P = OH * OW,
// K = Cin * k * k.  xp[n][ci][r][q] = x[n][ci][(r - hl) mod H][(q - wl) mod W] (the mathematical modulo; a pad may exceed the extent)
// is never written to memory: every kernel reads x at wrapped addresses.
//
// The matrix instruction: conv_tile.h states its lane maps, its k-ascending fmaf chain, which operand lies on the rows and which on
// the columns, the wave's pair of tiles and the rule that an operand outside its range is fed as +0; the helpers on the tile that
// this file shares with conv_transpose.hip are there too.
//
// Forward, one launch, a wave per (object, 32 channel pairs, 32 output pixels), four waves (128 pixels) per workgroup:
//   y[n][c2][oh][ow]: acc = b[c2]; for ci ASCENDING, kh ASCENDING, kw ASCENDING: acc = fmaf(xp[n][ci][oh*s + kh][ow*s + kw], w[c2][ci][kh][kw], acc)
//   TAIL: the instruction takes two k at a time; when K is odd one more step acc = fmaf(+0, +0, acc) closes the chain.  It changes
//   nothing but an accumulator of -0, which becomes +0 (K odd, b[c2] = -0 and every product -0).
//   a = y[c], b' = y[C + c]: first = a >= b' (a tie takes the first half, a NaN on either side the second); out = first ? a : b';
//   out [N][C][OH][OW] and one `first` byte (0 or 1) per output element are written, y is not.  An object's result does not depend on
//   the other objects of the call.
//
// Backward, cotangent g [N][C][OH][OW]: gy[c] = first ? g : +0, gy[C + c] = first ? +0 : g by SELECTION (an infinite cotangent gives
// (inf, 0)); gy is not written to memory.
//   Weight and bias gradient, two launches.  m = (n * OH + oh) * OW + ow < M = N * P; tap K of row c2 is the constant 1 (the bias):
//     t[c2][kk] = the sum over m of gy[m][c2] * (kk < K ? xp[m][kk] : 1)
//     CHUNK RULE: m is cut into chunks of kConvChunk = 1024 consecutive m (the last one shorter), a function of M alone.  Launch 1: per
//     chunk j one chain part[j][c2][kk], acc = +0, m ASCENDING: acc = fmaf(gy, xp, acc) (a chain from +0 is never -0, so the closing
//     fmaf(+0, +0, acc) of an odd chunk is invisible).  Launch 2: acc = part[0]; acc = acc + part[j] for j = 1, 2, .. ASCENDING, in fp32.
//     gw[c2][ci][kh][kw] = t[c2][kk], gb[c2] = t[c2][K].  Workspace: chunks * 2C * (K + 1) floats (ctpvae_conv_wgrad_workspace_bytes).
//     An unselected half contributes +0 * xp: +-0 for finite xp, NaN for a non-finite one.
//   Input gradient, one launch here and the fold of convblock.hip:
//     gp[n][ci][r][q]: acc = +0; for c2 ASCENDING, kh ASCENDING, kw ASCENDING: acc = fmaf(w[c2][ci][kh][kw], v, acc) with
//     v = gy[n][c2][(r - kh) / s][(q - kw) / s] where (r - kh) and (q - kw) are non-negative multiples of s with quotients below OH / OW,
//     and v = +0 at every other tap: an INVALID TAP ENTERS AS w * (+0) -- invisible for finite weights (a chain from +0 is never -0),
//     NaN for a non-finite weight.  gp [N][Cin][PH][PW] IS written to memory (the caller's buffer) and folded by
//     ctpvae_periodic_pad_bwd_f32 with its order: copies of a column ascending in q, then rows ascending in r.  The caller skips both
//     when x needs no gradient.
//
// Limits, refused with CTPVAE_EINVAL before any launch: 1 <= k <= 8, 1 <= s <= k, k <= PH, k <= PW, every element count (the tensors,
// gp, the workspace, the launches' workgroups) <= 2^31 - 1, null pointers.
#include <climits>

#include "common.h"
#include "conv_tile.h"

namespace ctpvae {

struct ConvGeom {
    int N, Cin, H, W, C, k, s;
    int PH, PW, OH, OW, P, K;          // P = OH * OW, K = Cin * k * k
    int sr0, sq0;                      // source row / column of padded row / column 0: (-hl) mod H, (-wl) mod W
    int sH, sW;                        // s mod H, s mod W
};

// out pixels on the columns, channel pairs on the rows; k runs over (ci, kh, kw)
__global__ __launch_bounds__(kConvThreads) void conv_fwd_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                                const float *__restrict__ b, ConvGeom gm, int ctiles, int pgroups,
                                                                float *__restrict__ out, unsigned char *__restrict__ first_out)
{
    const auto [wv, j, half] = tile_lane();
    int blk = blockIdx.x;
    const int pg = blk % pgroups;
    blk /= pgroups;
    const int ct = blk % ctiles, n = blk / ctiles;
    const int p = (pg * 4 + wv) * 32 + j;
    const bool pvalid = p < gm.P;
    const int oh = pvalid ? p / gm.OW : 0, ow = pvalid ? p - oh * gm.OW : 0;
    const int rr0 = (oh * gm.s + gm.sr0) % gm.H, cq0 = (ow * gm.s + gm.sq0) % gm.W;
    const int HW = gm.H * gm.W;
    int kh = 0, kw = 0, rr = rr0, cq = cq0, cbase = n * gm.Cin * HW;
    auto step = [&]() {
        ++kw, ++cq;
        if (cq == gm.W) cq = 0;
        if (kw == gm.k) {
            kw = 0, cq = cq0, ++kh, ++rr;
            if (rr == gm.H) rr = 0;
            if (kh == gm.k) kh = 0, rr = rr0, cbase += HW;
        }
    };
    if (half) step();
    const int c = ct * 32 + j;                         // this lane's ROW of the A operand
    const bool cvalid = c < gm.C;
    const float *wa = w + (size_t)(cvalid ? c : 0) * gm.K, *wb = w + (size_t)(cvalid ? gm.C + c : 0) * gm.K;
    f32x16 accA, accB;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const int cr = ct * 32 + tile_row(g, half);
        accA[g] = cr < gm.C ? b[cr] : 0.0f;
        accB[g] = cr < gm.C ? b[gm.C + cr] : 0.0f;
    }
    for (int kb = 0; kb < gm.K; kb += 2 * kConvDepth) {      // kb is wave-uniform: kConvDepth steps' operands in flight, then their MFMAs
        float xv[kConvDepth], a0[kConvDepth], a1[kConvDepth];
#pragma unroll
        for (int u = 0; u < kConvDepth; ++u) {
            const int kk = kb + 2 * u + half;
            const bool kvalid = kk < gm.K;
            xv[u] = kvalid && pvalid ? x[cbase + rr * gm.W + cq] : 0.0f;
            a0[u] = kvalid && cvalid ? wa[kk] : 0.0f;
            a1[u] = kvalid && cvalid ? wb[kk] : 0.0f;
            step();
            step();
        }
#pragma unroll
        for (int u = 0; u < kConvDepth; ++u)
            if (kb + 2 * u < gm.K) {                           // no step past the chain's end: the tail rule is one closing step at most
                accA = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], xv[u], accA, 0, 0, 0);
                accB = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u], xv[u], accB, 0, 0, 0);
            }
    }
    if (!pvalid) return;
    tile_store_maxout(accA, accB, ct, half, n, gm.C, gm.P, p, out, first_out);
}

// taps (and the bias's constant 1) on the columns, channel pairs on the rows; k runs over the m of one chunk
__global__ __launch_bounds__(kConvThreads) void conv_wgrad_kernel(const float *__restrict__ x, const float *__restrict__ g,
                                                                  const unsigned char *__restrict__ first_in, ConvGeom gm, int ctiles,
                                                                  int kgroups, int M, float *__restrict__ part)
{
    const auto [wv, j, half] = tile_lane();
    int blk = blockIdx.x;
    const int kg = blk % kgroups;
    blk /= kgroups;
    const int ct = blk % ctiles, chunk = blk / ctiles;
    const int kidx = (kg * 4 + wv) * 32 + j;
    if ((kg * 4 + wv) * 32 > gm.K) return;              // a whole wave past the last column (no barrier below)
    const bool kvalid = kidx < gm.K, isbias = kidx == gm.K;
    const int kk2 = gm.k * gm.k;
    const int ci = kvalid ? kidx / kk2 : 0, rem = kvalid ? kidx - ci * kk2 : 0, kh = rem / gm.k, kw = rem - kh * gm.k;
    const int rrbase = (kh + gm.sr0) % gm.H, cqbase = (kw + gm.sq0) % gm.W;
    int m_begin, m_end;
    chunk_range(chunk, M, m_begin, m_end);
    int m = m_begin + half;
    int n = m / gm.P, pix = m - n * gm.P, oh = pix / gm.OW, ow = pix - oh * gm.OW;
    int rr = (oh * gm.s + rrbase) % gm.H, cq = (ow * gm.s + cqbase) % gm.W;
    auto step = [&]() {
        ++pix, ++ow, cq += gm.sW;
        if (cq >= gm.W) cq -= gm.W;
        if (ow == gm.OW) {
            ow = 0, cq = cqbase, ++oh, rr += gm.sH;
            if (rr >= gm.H) rr -= gm.H;
            if (oh == gm.OH) oh = 0, pix = 0, rr = rrbase, ++n;
        }
    };
    const int c = ct * 32 + j;                          // this lane's ROW of the A operand
    const bool cvalid = c < gm.C;
    const int HW = gm.H * gm.W;
    f32x16 accA, accB;
    tile_zero(accA), tile_zero(accB);
    for (int mb = m_begin; mb < m_end; mb += 2 * kConvDepth) {   // mb is wave-uniform
        float gv[kConvDepth], xv[kConvDepth];
        unsigned char fb[kConvDepth];
#pragma unroll
        for (int u = 0; u < kConvDepth; ++u) {
            const bool mvalid = m + 2 * u < m_end;
            gv[u] = 0.0f, xv[u] = 0.0f, fb[u] = 0;
            if (mvalid && cvalid) {
                const size_t o = ((size_t)n * gm.C + c) * gm.P + pix;
                gv[u] = g[o], fb[u] = first_in[o];
            }
            if (mvalid) xv[u] = kvalid ? x[(n * gm.Cin + ci) * HW + rr * gm.W + cq] : (isbias ? 1.0f : 0.0f);
            step();
            step();
        }
        m += 2 * kConvDepth;
#pragma unroll
        for (int u = 0; u < kConvDepth; ++u)
            if (mb + 2 * u < m_end) tile_mfma_selected(accA, accB, fb[u] != 0, gv[u], xv[u]);
    }
    if (kidx > gm.K) return;
    const size_t row = (size_t)gm.K + 1, base = (size_t)chunk * 2 * gm.C;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int cr = ct * 32 + tile_row(r, half);
        if (cr < gm.C) {
            part[(base + cr) * row + kidx] = accA[r];
            part[(base + gm.C + cr) * row + kidx] = accB[r];
        }
    }
}

// one thread per element of [2C][K + 1]: the chunks' partials in ascending order
__global__ __launch_bounds__(kConvThreads) void conv_wgrad_finish_kernel(const float *__restrict__ part, int chunks, int C2, int K,
                                                                         float *__restrict__ gw, float *__restrict__ gb)
{
    const unsigned total = (unsigned)C2 * (unsigned)(K + 1);
    const unsigned e = blockIdx.x * kConvThreads + threadIdx.x;
    if (e >= total) return;
    const float acc = chunk_sum(part, chunks, total, e);
    const unsigned c2 = e / (unsigned)(K + 1), kidx = e - c2 * (unsigned)(K + 1);
    if (kidx < (unsigned)K) gw[(size_t)c2 * K + kidx] = acc;
    else gb[c2] = acc;
}

// padded pixels on the columns, input channels on the rows; k runs over (c2, kh, kw).  ONE tile per wave (there is no pair here).
__global__ __launch_bounds__(kConvThreads) void conv_dgrad_kernel(const float *__restrict__ g, const unsigned char *__restrict__ first_in,
                                                                  const float *__restrict__ w, ConvGeom gm, int citiles, int pgroups,
                                                                  float *__restrict__ gp)
{
    __shared__ int tab[4][2][kConvMaxK][32];            // per wave: [0][kh][j] = oh * OW or -1, [1][kw][j] = ow or -1
    const auto [wv, j, half] = tile_lane();
    int blk = blockIdx.x;
    const int pg = blk % pgroups;
    blk /= pgroups;
    const int cit = blk % citiles, n = blk / citiles;
    const int PP = gm.PH * gm.PW;
    const int p = (pg * 4 + wv) * 32 + j;
    const bool pvalid = p < PP;
    const int r = pvalid ? p / gm.PW : 0, q = pvalid ? p - r * gm.PW : 0;
    {
        const int v = half ? q : r, lim = half ? gm.OW : gm.OH, mul = half ? 1 : gm.OW;
        for (int t = 0; t < gm.k; ++t) {
            const int d = v - t, quo = d >= 0 ? d / gm.s : 0;
            tab[wv][half][t][j] = pvalid && d >= 0 && quo * gm.s == d && quo < lim ? quo * mul : -1;
        }
    }
    __syncthreads();
    const int kk2 = gm.k * gm.k, K2 = 2 * gm.C * kk2;
    int c2 = 0, kh = 0, kw = 0;
    auto step = [&]() {
        if (++kw == gm.k) {
            kw = 0;
            if (++kh == gm.k) kh = 0, ++c2;
        }
    };
    if (half) step();
    const int ci = cit * 32 + j;                        // this lane's ROW of the A operand
    const bool civalid = ci < gm.Cin;
    f32x16 acc;
    tile_zero(acc);
    for (int kb = 0; kb < K2; kb += 2 * kConvDepth) {         // kb is wave-uniform
        float gv[kConvDepth], wv_[kConvDepth];
        unsigned char take[kConvDepth];                        // 1: the cotangent goes to this c2's half
#pragma unroll
        for (int u = 0; u < kConvDepth; ++u) {
            gv[u] = 0.0f, wv_[u] = 0.0f, take[u] = 0;
            if (kb + 2 * u + half < K2) {
                const int ro = tab[wv][0][kh][j], co = tab[wv][1][kw][j];
                if (ro >= 0 && co >= 0) {
                    const bool second = c2 >= gm.C;
                    const size_t o = ((size_t)n * gm.C + (second ? c2 - gm.C : c2)) * gm.P + ro + co;
                    gv[u] = g[o];
                    take[u] = (first_in[o] != 0) != second ? 1 : 0;
                }
                if (civalid) wv_[u] = w[((size_t)c2 * gm.Cin + ci) * kk2 + kh * gm.k + kw];
            }
            step();
            step();
        }
#pragma unroll
        for (int u = 0; u < kConvDepth; ++u)
            if (kb + 2 * u < K2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv_[u], take[u] ? gv[u] : 0.0f, acc, 0, 0, 0);
    }
    if (!pvalid) return;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int cr = cit * 32 + tile_row(t, half);
        if (cr < gm.Cin) gp[((size_t)n * gm.Cin + cr) * PP + p] = acc[t];
    }
}

static int conv_check(const char *what, int N, int Cin, int H, int W, int C, int k, int s, int wl, int wr, int hl, int hr, ConvGeom *gm)
{
    if (int rc = conv_check_common(what, N, Cin, H, W, C, k, s)) return rc;
    CTPVAE_REQUIRE(wl >= 0 && wr >= 0 && hl >= 0 && hr >= 0, "%s: pads must not be negative (wl=%d wr=%d hl=%d hr=%d)", what, wl, wr, hl, hr);
    const long long PH = (long long)H + hl + hr, PW = (long long)W + wl + wr;
    CTPVAE_REQUIRE(PH >= k && PW >= k, "%s: the padded image (%lld x %lld) must hold one window of %d x %d", what, PH, PW, k, k);
    const long long OH = (PH - k) / s + 1, OW = (PW - k) / s + 1, P = OH * OW, K = (long long)Cin * k * k;
    const long long lim = INT_MAX;
    CTPVAE_REQUIRE(PH <= lim && PW <= lim && PH * PW <= lim && (long long)N * Cin <= lim && (long long)N * Cin * (PH * PW) <= lim,
                   "%s: N * Cin * PH * PW must fit 31 bits (N=%d Cin=%d, %lld x %lld)", what, N, Cin, PH, PW);
    CTPVAE_REQUIRE((long long)H * W <= lim && (long long)N * Cin * ((long long)H * W) <= lim, "%s: N * Cin * H * W must fit 31 bits", what);
    CTPVAE_REQUIRE(C <= lim / 2 && P <= lim && (long long)N * P <= lim && 2ll * C * ((long long)N * P) <= lim,
                   "%s: N * 2C * OH * OW must fit 31 bits (N=%d C=%d, %lld x %lld)", what, N, C, OH, OW);
    CTPVAE_REQUIRE(K < lim && 2ll * C * (K + 1) <= lim, "%s: 2C * (Cin * k * k + 1) must fit 31 bits (C=%d Cin=%d k=%d)", what, C, Cin, k);
    *gm = ConvGeom{N, Cin, H, W, C, k, s, (int)PH, (int)PW, (int)OH, (int)OW, (int)P, (int)K,
                   (H - hl % H) % H, (W - wl % W) % W, s % H, s % W};
    return CTPVAE_OK;
}

// chunks of the weight gradient and the floats of its workspace; -1 when the workspace's element count does not fit 31 bits
static long long conv_wgrad_floats(const ConvGeom &gm, int *chunks)
{
    const long long M = (long long)gm.N * gm.P, ch = ceil_div(M, kConvChunk), fl = ch * 2 * gm.C * ((long long)gm.K + 1);
    *chunks = (int)ch;
    return fl <= INT_MAX ? fl : -1;
}

}  // namespace ctpvae

using namespace ctpvae;

extern "C" {

int ctpvae_conv_wgrad_chunk_len(void) { return kConvChunk; }

long long ctpvae_conv_wgrad_workspace_bytes(int N, int Cin, int H, int W, int C, int k, int s, int wl, int wr, int hl, int hr)
{
    ConvGeom gm;
    if (int rc = conv_check("conv_wgrad_workspace_bytes", N, Cin, H, W, C, k, s, wl, wr, hl, hr, &gm)) return rc;
    int chunks;
    const long long fl = conv_wgrad_floats(gm, &chunks);
    CTPVAE_REQUIRE(fl >= 0, "conv_wgrad_workspace_bytes: chunks * 2C * (K + 1) must fit 31 bits (chunks=%d C=%d K=%d)", chunks, C, gm.K);
    return fl * 4;
}

int ctpvae_conv_fwd_f32(const float *x_dev, const float *w_dev, const float *b_dev, int N, int Cin, int H, int W, int C, int k, int s, int wl,
                        int wr, int hl, int hr, float *out_dev, unsigned char *first_out_dev, ctpvae_stream_t stream)
{
    CTPVAE_REQUIRE(x_dev && w_dev && b_dev && out_dev && first_out_dev, "conv_fwd: null pointer");
    ConvGeom gm;
    if (int rc = conv_check("conv_fwd", N, Cin, H, W, C, k, s, wl, wr, hl, hr, &gm)) return rc;
    const long long ctiles = ceil_div(C, 32), pgroups = ceil_div(gm.P, 128), blocks = (long long)N * ctiles * pgroups;
    if (int rc = conv_check_blocks("conv_fwd", blocks)) return rc;
    hipLaunchKernelGGL(conv_fwd_kernel, dim3((unsigned)blocks), dim3(kConvThreads), 0, (hipStream_t)stream, x_dev, w_dev, b_dev, gm,
                       (int)ctiles, (int)pgroups, out_dev, first_out_dev);
    CTPVAE_LAUNCH_CHECK("conv_fwd_kernel");
    return CTPVAE_OK;
}

int ctpvae_conv_bwd_weight_f32(const float *x_dev, const float *g_dev, const unsigned char *first_dev, int N, int Cin, int H, int W, int C,
                               int k, int s, int wl, int wr, int hl, int hr, void *workspace_dev, float *gw_out_dev, float *gb_out_dev,
                               ctpvae_stream_t stream)
{
    CTPVAE_REQUIRE(x_dev && g_dev && first_dev && workspace_dev && gw_out_dev && gb_out_dev, "conv_bwd_weight: null pointer");
    ConvGeom gm;
    if (int rc = conv_check("conv_bwd_weight", N, Cin, H, W, C, k, s, wl, wr, hl, hr, &gm)) return rc;
    int chunks;
    CTPVAE_REQUIRE(conv_wgrad_floats(gm, &chunks) >= 0, "conv_bwd_weight: chunks * 2C * (K + 1) must fit 31 bits (chunks=%d C=%d K=%d)",
                   chunks, C, gm.K);
    const long long ctiles = ceil_div(C, 32), kgroups = ceil_div((long long)gm.K + 1, 128), blocks = chunks * ctiles * kgroups;
    if (int rc = conv_check_blocks("conv_bwd_weight", blocks)) return rc;
    hipLaunchKernelGGL(conv_wgrad_kernel, dim3((unsigned)blocks), dim3(kConvThreads), 0, (hipStream_t)stream, x_dev, g_dev, first_dev, gm,
                       (int)ctiles, (int)kgroups, N * gm.P, (float *)workspace_dev);
    CTPVAE_LAUNCH_CHECK("conv_wgrad_kernel");
    const unsigned total = 2u * (unsigned)C * (unsigned)(gm.K + 1);
    hipLaunchKernelGGL(conv_wgrad_finish_kernel, dim3((total + kConvThreads - 1) / kConvThreads), dim3(kConvThreads), 0, (hipStream_t)stream,
                       (const float *)workspace_dev, chunks, 2 * C, gm.K, gw_out_dev, gb_out_dev);
    CTPVAE_LAUNCH_CHECK("conv_wgrad_finish_kernel");
    return CTPVAE_OK;
}

int ctpvae_conv_bwd_input_f32(const float *g_dev, const unsigned char *first_dev, const float *w_dev, int N, int Cin, int H, int W, int C,
                              int k, int s, int wl, int wr, int hl, int hr, float *gp_out_dev, ctpvae_stream_t stream)
{
    CTPVAE_REQUIRE(g_dev && first_dev && w_dev && gp_out_dev, "conv_bwd_input: null pointer");
    ConvGeom gm;
    if (int rc = conv_check("conv_bwd_input", N, Cin, H, W, C, k, s, wl, wr, hl, hr, &gm)) return rc;
    const long long citiles = ceil_div(Cin, 32), pgroups = ceil_div((long long)gm.PH * gm.PW, 128), blocks = (long long)N * citiles * pgroups;
    if (int rc = conv_check_blocks("conv_bwd_input", blocks)) return rc;
    hipLaunchKernelGGL(conv_dgrad_kernel, dim3((unsigned)blocks), dim3(kConvThreads), 0, (hipStream_t)stream, g_dev, first_dev, w_dev, gm,
                       (int)citiles, (int)pgroups, gp_out_dev);
    CTPVAE_LAUNCH_CHECK("conv_dgrad_kernel");
    return CTPVAE_OK;
}

}  // extern "C"
