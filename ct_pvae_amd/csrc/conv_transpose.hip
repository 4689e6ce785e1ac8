// conv_transpose.hip -- the transposed convolution of an up-sampling ConvBlock (ctvae/models.py:267-342, Conv2DTranspose; ct_pvae_amd/
// trainer.py ConvBlock with transpose=True) with its maxout behind, as ONE forward launch and at most three backward launches, on the
// matrix cores with fp32 operands (v_mfma_f32_32x32x2_f32; conv_tile.h states the instruction's lane maps and its chain and holds
// the constants and the helpers on the tile that this file shares with conv.hip).  Every sum has ONE stated order; no atomics;
// nothing depends on the device, its CU count, a knob or launch-time state; tests/np_twin_conv_transpose.py restates this header and
// the kernels are held to it BY BITS.
//
// Operands, all contiguous fp32: x [N][Cin][H][W], w [Cin][2C][k][k] (nn.ConvTranspose2d's weight, read where the module keeps it; the
// maxout's halves are the ranges [0, C) and [C, 2C) of axis 1), b [2C], stride s, padding pad, output padding opad.
// OH = (H - 1) * s - 2 * pad + k + opad, OW likewise, P = OH * OW.  For output row oy let t = oy + pad: tap kh reaches source row
// iy = (t - kh) / s, and only where s divides t - kh; columns likewise.
//
// Forward, one launch.  The PHASE taps of an output pixel are the kh = (oy + pad) mod s, + s, + 2s .. < k (Th of them) and the kw
// likewise (Tw); taps of other phases are not in the chain and no instruction is spent on them.  Output pixels of ONE phase
// (py, px) = ((oy + pad) mod s, (ox + pad) mod s) lie on the columns, row-major over the phase's rows and columns, so the k loop is
// wave-uniform and consecutive columns read consecutive ix; channel pairs lie on the rows, a wave computes the two halves' tiles over
// the shared column operand; four waves (128 pixels of a phase) per workgroup, a workgroup per (object, 32 channel pairs, phase, 128
// pixels); loads are issued kConvDepth steps ahead of their instructions, and every operand load of the file is branch-free
// (load_or_zero), so the loads of a group are in flight together.  Operands come straight from global memory through the caches;
// there is no LDS staging.
//   y[n][c2][oy][ox]: acc = b[c2]; for ci ASCENDING, phase kh ASCENDING, phase kw ASCENDING: acc = fmaf(v, w[ci][c2][kh][kw], acc) with
//   v = x[n][ci][iy][ix] where 0 <= iy < H and 0 <= ix < W and v = +0 at a phase tap that falls outside the image (the image's edge
//   and the opad rows and columns produce such taps).
//   TAIL: when the chain's length Cin * Th * Tw is odd, one closing acc = fmaf(+0, +0, acc) follows (it turns an accumulator of -0
//   into +0 and changes nothing else).  The parity may differ between the phases of one call (k = 3, s = 2: 1, 2 or 4 taps).
//   a = y[c], b' = y[C + c]: first = a >= b' (a tie takes the first half, a NaN on either side the second); out = first ? a : b';
//   out [N][C][OH][OW] and one `first` byte (0 or 1) per output element are written, y is not.  An object's result does not depend on
//   the other objects of the call.
//
// Backward, cotangent g [N][C][OH][OW]: gy[c] = first ? g : +0, gy[C + c] = first ? +0 : g by SELECTION (an infinite cotangent gives
// (inf, 0)); gy is not written to memory.
//   Input gradient, one launch, written straight to gx [N][Cin][H][W] (there is no pad to fold); input channels on the rows, input
//   pixels on the columns, one tile per wave:
//     gx[n][ci][iy][ix]: acc = +0; for c2 ASCENDING, kh ASCENDING, kw ASCENDING: acc = fmaf(w[ci][c2][kh][kw], v, acc) with
//     v = gy[n][c2][iy * s - pad + kh][ix * s - pad + kw], or +0 where that position is outside [0, OH) x [0, OW): an INVALID TAP ENTERS AS
//     w * (+0) -- invisible for finite weights (a chain from +0 is never -0), NaN for a non-finite one.  2C * k * k is even: no tail.
//   Weight and bias gradient, two launches.
//     gw[ci][c2][kh][kw] = the sum over m of x[m][ci] * gy_tap[m][c2], m = (n * H + iy) * W + ix < M = N * H * W, gy_tap the selected
//     cotangent at (iy * s - pad + kh, ix * s - pad + kw); A POSITION OUTSIDE THE OUTPUT ENTERS AS +0, so a non-finite x there gives NaN.
//     CHUNK RULE: m is cut into chunks of kConvChunk = 1024 consecutive m (the last one shorter), a function of M alone
//     (ctpvae_conv_wgrad_chunk_len).  Per chunk one chain from +0, m ASCENDING: acc = fmaf(gy_tap, x, acc) (a chain from +0 is never -0,
//     so the closing step of an odd chunk is invisible).  The tap fixes the row operand, so a tile -- one wave -- is one (chunk, tap,
//     32 channel pairs, 32 ci): channel pairs on the rows, ci on the columns.
//     gb[c2] = the sum of gy over mo = (n * OH + oy) * OW + ox < Mo = N * P (the input-pixel walk cannot carry it: taps cover output
//     pixels unevenly): chunks of 1024 consecutive mo, per chunk one chain from +0, mo ASCENDING, acc = fmaf(gy, 1, acc), which is
//     plain fp32 addition.  These chains are further waves of the first weight launch (the column operand is the constant 1).
//     The finishing launch adds the partials of gw and of gb in ascending chunk order in fp32, starting from the first.
//     Workspace: chunks(M) * Cin * 2C * k * k + chunks(Mo) * 2C floats (ctpvae_convt_wgrad_workspace_bytes).
//
// Limits, refused with CTPVAE_EINVAL before any launch: every extent >= 1, 1 <= k <= 8, 1 <= s <= k, 0 <= pad < k, 0 <= opad < s,
// OH >= 1, OW >= 1, every element count (the tensors with 2C channels, the workspace, the launches' workgroups) <= 2^31 - 1, null
// pointers.
#include <climits>

#include "common.h"
#include "conv_tile.h"

namespace ctpvae {

// Steps of the two backward kernels' k loops per group.  Their chains are long and their waves few (a chunk of 1024 m, or 2C * k * k
// taps, per wave), so a group's loads are issued one whole group ahead: the NEXT group's loads are in flight during this group's
// MFMAs.  Like kConvDepth it has no effect on any result.
constexpr int kConvtDepth = 16;

struct ConvtGeom {
    int N, Cin, H, W, C, k, s, pad;
    int OH, OW, P, HW;                 // P = OH * OW, HW = H * W
};

// the first output index of phase ph along an axis: the smallest o >= 0 with (o + pad) mod s == ph
__device__ __forceinline__ int convt_phase_first(int ph, int pad, int s) { return ((ph - pad) % s + s) % s; }

// output pixels of one phase on the columns, channel pairs on the rows; k runs over (ci, phase kh, phase kw)
__global__ __launch_bounds__(kConvThreads) void convt_fwd_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                                 const float *__restrict__ b, ConvtGeom gm, int ctiles, int pgroups,
                                                                 float *__restrict__ out, unsigned char *__restrict__ first_out)
{
    const auto [wv, j, half] = tile_lane();
    int blk = blockIdx.x;
    const int pg = blk % pgroups;
    blk /= pgroups;
    const int phase = blk % (gm.s * gm.s);
    blk /= gm.s * gm.s;
    const int ct = blk % ctiles, n = blk / ctiles;
    const int py = phase / gm.s, px = phase - py * gm.s;
    const int oy0 = convt_phase_first(py, gm.pad, gm.s), ox0 = convt_phase_first(px, gm.pad, gm.s);
    const int RH = oy0 < gm.OH ? (gm.OH - 1 - oy0) / gm.s + 1 : 0, RW = ox0 < gm.OW ? (gm.OW - 1 - ox0) / gm.s + 1 : 0;
    if ((pg * 4 + wv) * 32 >= RH * RW) return;          // a whole wave past the phase's last pixel (no barrier below)
    const int Th = (gm.k - 1 - py) / gm.s + 1, Tw = (gm.k - 1 - px) / gm.s + 1, L = gm.Cin * Th * Tw;
    const int pp = (pg * 4 + wv) * 32 + j;
    const bool pvalid = pp < RH * RW;
    const int r = pvalid ? pp / RW : 0, cc = pvalid ? pp - r * RW : 0;
    const int iy0 = (oy0 + gm.pad - py) / gm.s + r, ix0 = (ox0 + gm.pad - px) / gm.s + cc;      // the source of tap (a, b) is (iy0 - a, ix0 - b)
    const int kk2 = gm.k * gm.k, C2 = 2 * gm.C;
    int ci = 0, a = 0, bq = 0;
    auto step = [&]() {
        if (++bq == Tw) {
            bq = 0;
            if (++a == Th) a = 0, ++ci;
        }
    };
    if (half) step();
    const int c = ct * 32 + j;                          // this lane's ROW of the A operand
    const bool cvalid = c < gm.C;
    const int wa0 = (cvalid ? c : 0) * kk2 + py * gm.k + px, wb0 = wa0 + (cvalid ? gm.C * kk2 : 0);
    f32x16 accA, accB;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const int cr = ct * 32 + tile_row(g, half);
        accA[g] = load_or_zero(b, cr < gm.C, (size_t)cr);
        accB[g] = load_or_zero(b, cr < gm.C, (size_t)(gm.C + cr));
    }
    for (int kb = 0; kb < L; kb += 2 * kConvDepth) {    // kb is wave-uniform: kConvDepth steps' operands in flight, then their MFMAs
        float xv[kConvDepth], a0[kConvDepth], a1[kConvDepth];
#pragma unroll
        for (int u = 0; u < kConvDepth; ++u) {
            const bool kvalid = kb + 2 * u + half < L;
            const int iy = iy0 - a, ix = ix0 - bq;
            const bool inside = iy >= 0 && iy < gm.H && ix >= 0 && ix < gm.W;
            xv[u] = load_or_zero(x, kvalid && pvalid && inside, (size_t)((n * gm.Cin + ci) * gm.HW + iy * gm.W + ix));
            const int wo = ci * C2 * kk2 + gm.s * (a * gm.k + bq);
            a0[u] = load_or_zero(w, kvalid && cvalid, (size_t)(wa0 + wo));
            a1[u] = load_or_zero(w, kvalid && cvalid, (size_t)(wb0 + wo));
            step();
            step();
        }
#pragma unroll
        for (int u = 0; u < kConvDepth; ++u)
            if (kb + 2 * u < L) {                       // no step past the chain's end: the tail rule is one closing step at most
                accA = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], xv[u], accA, 0, 0, 0);
                accB = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u], xv[u], accB, 0, 0, 0);
            }
    }
    if (!pvalid) return;
    const int oy = oy0 + gm.s * r, ox = ox0 + gm.s * cc;
    tile_store_maxout(accA, accB, ct, half, n, gm.C, gm.P, oy * gm.OW + ox, out, first_out);
}

// input pixels on the columns, input channels on the rows; k runs over (c2, kh, kw).  ONE tile per wave (there is no pair here).
__global__ __launch_bounds__(kConvThreads) void convt_dgrad_kernel(const float *__restrict__ g, const unsigned char *__restrict__ first_in,
                                                                   const float *__restrict__ w, ConvtGeom gm, int citiles, int pgroups,
                                                                   float *__restrict__ gx)
{
    const auto [wv, j, half] = tile_lane();
    int blk = blockIdx.x;
    const int pg = blk % pgroups;
    blk /= pgroups;
    const int cit = blk % citiles, n = blk / citiles;
    if ((pg * 4 + wv) * 32 >= gm.HW) return;            // a whole wave past the last pixel (no barrier below)
    const int p = (pg * 4 + wv) * 32 + j;
    const bool pvalid = p < gm.HW;
    const int iy = pvalid ? p / gm.W : 0, ix = pvalid ? p - iy * gm.W : 0;
    const int oyb = iy * gm.s - gm.pad, oxb = ix * gm.s - gm.pad;
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
    const float *wr = w + (size_t)(civalid ? ci : 0) * K2;      // w[ci][c2][kh][kw]: the chain's index is the offset
    f32x16 acc;
    tile_zero(acc);
    int left = K2 - half;                               // steps of the chain from this lane's next one on (it may fall below 0)
    auto fetch = [&](float (&gq)[kConvtDepth], float (&wq)[kConvtDepth], unsigned char (&tq)[kConvtDepth]) {
#pragma unroll
        for (int u = 0; u < kConvtDepth; ++u) {
            const bool kvalid = 2 * u < left, second = c2 >= gm.C;
            const int oy = oyb + kh, ox = oxb + kw;
            const bool inside = kvalid && pvalid && oy >= 0 && oy < gm.OH && ox >= 0 && ox < gm.OW;
            const size_t o = ((size_t)n * gm.C + (second ? c2 - gm.C : c2)) * gm.P + oy * gm.OW + ox;
            gq[u] = load_or_zero(g, inside, o);
            tq[u] = (unsigned char)(inside & ((load_or_zero(first_in, inside, o) != 0) != second));
            wq[u] = load_or_zero(wr, kvalid && civalid, (size_t)(K2 - left + 2 * u));      // K2 - left: this lane's next step of the chain
            step();
            step();
        }
        left -= 2 * kConvtDepth;
    };
    float gv[kConvtDepth], wv_[kConvtDepth];
    unsigned char take[kConvtDepth];                     // 1: the cotangent goes to this c2's half
    fetch(gv, wv_, take);
    for (int todo = K2; todo > 0; todo -= 2 * kConvtDepth) {    // todo is wave-uniform
        float gn[kConvtDepth], wn[kConvtDepth];
        unsigned char tn[kConvtDepth];
        fetch(gn, wn, tn);                               // the next group's (past the chain's end: no load, +0)
#pragma unroll
        for (int u = 0; u < kConvtDepth; ++u)
            if (2 * u < todo) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv_[u], take[u] ? gv[u] : 0.0f, acc, 0, 0, 0);
#pragma unroll
        for (int u = 0; u < kConvtDepth; ++u) gv[u] = gn[u], wv_[u] = wn[u], take[u] = tn[u];
    }
    if (!pvalid) return;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int cr = cit * 32 + tile_row(t, half);
        if (cr < gm.Cin) gx[((size_t)n * gm.Cin + cr) * gm.HW + p] = acc[t];
    }
}

// A wave per tile.  Workgroups below wblocks: the weight gradient's (chunk, channel-pair tile, ci tile, tap), the tap fastest, with the
// selected cotangent at the tap's shift on the rows, x[m][ci] on the columns and k over the m of the chunk.  Workgroups from wblocks:
// the bias gradient's (chunk of mo, channel-pair tile): the same walk over the OUTPUT pixels with no shift and the constant 1 on the
// columns, of which column 0 is stored.
__global__ __launch_bounds__(kConvThreads) void convt_wgrad_kernel(const float *__restrict__ x, const float *__restrict__ g,
                                                                   const unsigned char *__restrict__ first_in, ConvtGeom gm, int ctiles,
                                                                   int citiles, int wwaves, int wblocks, int bwaves, int M, int Mo,
                                                                   float *__restrict__ part, float *__restrict__ partb)
{
    const auto [wv, j, half] = tile_lane();
    const bool isbias = (int)blockIdx.x >= wblocks;
    const int kk2 = gm.k * gm.k;
    int wid = ((int)blockIdx.x - (isbias ? wblocks : 0)) * 4 + wv;
    if (wid >= (isbias ? bwaves : wwaves)) return;      // a whole wave past the last tile (no barrier below)
    int tap = 0, cit = 0;
    if (!isbias) {
        tap = wid % kk2, wid /= kk2;
        cit = wid % citiles, wid /= citiles;
    }
    const int ct = wid % ctiles, chunk = wid / ctiles;
    // the walk: rows x columns of the walked image, and the output position of a walked pixel (wy, wx) is (wy * st + offy, wx * st + offx)
    const int WH = isbias ? gm.OH : gm.H, WW = isbias ? gm.OW : gm.W, st = isbias ? 1 : gm.s;
    const int kh = tap / gm.k, offy = isbias ? 0 : kh - gm.pad, offx = isbias ? 0 : tap - kh * gm.k - gm.pad;
    int m_begin, m_end;
    chunk_range(chunk, isbias ? Mo : M, m_begin, m_end);
    int m = m_begin + half;
    int n = m / (WH * WW), wy = (m - n * (WH * WW)) / WW, wx = m - n * (WH * WW) - wy * WW;
    auto step = [&]() {
        if (++wx == WW) {
            wx = 0;
            if (++wy == WH) wy = 0, ++n;
        }
    };
    const int c = ct * 32 + j;                          // this lane's ROW of the A operand
    const bool cvalid = c < gm.C;
    const int ci = cit * 32 + j;                        // this lane's COLUMN of the B operand
    const bool civalid = ci < gm.Cin;
    f32x16 accA, accB;
    tile_zero(accA), tile_zero(accB);
    int left = m_end - m;                               // steps of the chunk from this lane's next one on (it may fall below 0)
    auto fetch = [&](float (&gq)[kConvtDepth], float (&xq)[kConvtDepth], unsigned char (&fq)[kConvtDepth]) {
#pragma unroll
        for (int u = 0; u < kConvtDepth; ++u) {
            const bool mvalid = 2 * u < left;
            const int oy = wy * st + offy, ox = wx * st + offx;
            const bool inside = mvalid && cvalid && oy >= 0 && oy < gm.OH && ox >= 0 && ox < gm.OW;
            const size_t o = ((size_t)n * gm.C + c) * gm.P + oy * gm.OW + ox;
            gq[u] = load_or_zero(g, inside, o), fq[u] = load_or_zero(first_in, inside, o);
            const float xl = load_or_zero(x, mvalid && civalid && !isbias, (size_t)((n * gm.Cin + ci) * gm.HW + wy * gm.W + wx));
            xq[u] = isbias ? (mvalid ? 1.0f : 0.0f) : xl;
            step();
            step();
        }
        left -= 2 * kConvtDepth;
    };
    float gv[kConvtDepth], xv[kConvtDepth];
    unsigned char fb[kConvtDepth];
    fetch(gv, xv, fb);
    for (int todo = m_end - m_begin; todo > 0; todo -= 2 * kConvtDepth) {   // todo is wave-uniform
        float gn[kConvtDepth], xn[kConvtDepth];
        unsigned char fn[kConvtDepth];
        fetch(gn, xn, fn);                               // the next group's (past the chunk's end: no load, +0)
#pragma unroll
        for (int u = 0; u < kConvtDepth; ++u)
            if (2 * u < todo) tile_mfma_selected(accA, accB, fb[u] != 0, gv[u], xv[u]);
#pragma unroll
        for (int u = 0; u < kConvtDepth; ++u) gv[u] = gn[u], xv[u] = xn[u], fb[u] = fn[u];
    }
    const int C2 = 2 * gm.C;
    if (isbias) {
        if (j != 0) return;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int cr = ct * 32 + tile_row(r, half);
            if (cr < gm.C) {
                partb[(size_t)chunk * C2 + cr] = accA[r];
                partb[(size_t)chunk * C2 + gm.C + cr] = accB[r];
            }
        }
        return;
    }
    if (!civalid) return;
    const size_t base = ((size_t)chunk * gm.Cin + ci) * C2;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int cr = ct * 32 + tile_row(r, half);
        if (cr < gm.C) {
            part[(base + cr) * kk2 + tap] = accA[r];
            part[(base + gm.C + cr) * kk2 + tap] = accB[r];
        }
    }
}

// one thread per element of gw [Cin][2C][k][k], then of gb [2C]: the chunks' partials in ascending order
__global__ __launch_bounds__(kConvThreads) void convt_wgrad_finish_kernel(const float *__restrict__ part, const float *__restrict__ partb,
                                                                          int chunks, int chunks_o, unsigned totalw, unsigned C2,
                                                                          float *__restrict__ gw, float *__restrict__ gb)
{
    const unsigned e = blockIdx.x * kConvThreads + threadIdx.x;
    if (e >= totalw + C2) return;
    if (e < totalw) gw[e] = chunk_sum(part, chunks, totalw, e);
    else gb[e - totalw] = chunk_sum(partb, chunks_o, C2, e - totalw);
}

static int convt_check(const char *what, int N, int Cin, int H, int W, int C, int k, int s, int pad, int opad, ConvtGeom *gm)
{
    if (int rc = conv_check_common(what, N, Cin, H, W, C, k, s)) return rc;
    CTPVAE_REQUIRE(pad >= 0 && pad < k, "%s: the padding must be in 0 .. k - 1 (got pad=%d k=%d)", what, pad, k);
    CTPVAE_REQUIRE(opad >= 0 && opad < s, "%s: the output padding must be in 0 .. s - 1 (got opad=%d s=%d)", what, opad, s);
    const long long OH = ((long long)H - 1) * s - 2 * pad + k + opad, OW = ((long long)W - 1) * s - 2 * pad + k + opad, P = OH * OW;
    CTPVAE_REQUIRE(OH >= 1 && OW >= 1, "%s: the output (%lld x %lld) must have at least one pixel", what, OH, OW);
    const long long lim = INT_MAX;
    CTPVAE_REQUIRE((long long)H * W <= lim && (long long)N * Cin <= lim && (long long)N * Cin * ((long long)H * W) <= lim,
                   "%s: N * Cin * H * W must fit 31 bits (N=%d Cin=%d H=%d W=%d)", what, N, Cin, H, W);
    CTPVAE_REQUIRE(C <= lim / 2 && OH <= lim && OW <= lim && P <= lim && (long long)N * P <= lim && 2ll * C * ((long long)N * P) <= lim,
                   "%s: N * 2C * OH * OW must fit 31 bits (N=%d C=%d, %lld x %lld)", what, N, C, OH, OW);
    CTPVAE_REQUIRE(2ll * C * k * k <= lim && (long long)Cin * (2ll * C * k * k) <= lim, "%s: Cin * 2C * k * k must fit 31 bits (Cin=%d C=%d k=%d)",
                   what, Cin, C, k);
    *gm = ConvtGeom{N, Cin, H, W, C, k, s, pad, (int)OH, (int)OW, (int)P, H * W};
    return CTPVAE_OK;
}

// chunks of the weight and of the bias gradient and the floats of their workspace; -1 when that count does not fit 31 bits
static long long convt_wgrad_floats(const ConvtGeom &gm, int *chunks, int *chunks_o)
{
    const long long ch = ceil_div((long long)gm.N * gm.HW, kConvChunk), cho = ceil_div((long long)gm.N * gm.P, kConvChunk);
    const long long fl = ch * gm.Cin * 2 * gm.C * gm.k * gm.k + cho * 2 * gm.C;
    *chunks = (int)ch, *chunks_o = (int)cho;
    return fl <= INT_MAX ? fl : -1;
}

}  // namespace ctpvae

using namespace ctpvae;

extern "C" {

long long ctpvae_convt_wgrad_workspace_bytes(int N, int Cin, int H, int W, int C, int k, int s, int pad, int opad)
{
    ConvtGeom gm;
    if (int rc = convt_check("convt_wgrad_workspace_bytes", N, Cin, H, W, C, k, s, pad, opad, &gm)) return rc;
    int chunks, chunks_o;
    const long long fl = convt_wgrad_floats(gm, &chunks, &chunks_o);
    CTPVAE_REQUIRE(fl >= 0, "convt_wgrad_workspace_bytes: chunks * Cin * 2C * k * k + output chunks * 2C must fit 31 bits (chunks=%d and %d "
                   "Cin=%d C=%d k=%d)", chunks, chunks_o, Cin, C, k);
    return fl * 4;
}

int ctpvae_convt_fwd_f32(const float *x_dev, const float *w_dev, const float *b_dev, int N, int Cin, int H, int W, int C, int k, int s, int pad,
                         int opad, float *out_dev, unsigned char *first_out_dev, ctpvae_stream_t stream)
{
    CTPVAE_REQUIRE(x_dev && w_dev && b_dev && out_dev && first_out_dev, "convt_fwd: null pointer");
    ConvtGeom gm;
    if (int rc = convt_check("convt_fwd", N, Cin, H, W, C, k, s, pad, opad, &gm)) return rc;
    const long long ctiles = ceil_div(C, 32), pgroups = ceil_div(ceil_div(gm.OH, s) * ceil_div(gm.OW, s), 128);
    const long long blocks = (long long)N * ctiles * s * s * pgroups;
    if (int rc = conv_check_blocks("convt_fwd", blocks)) return rc;
    hipLaunchKernelGGL(convt_fwd_kernel, dim3((unsigned)blocks), dim3(kConvThreads), 0, (hipStream_t)stream, x_dev, w_dev, b_dev, gm,
                       (int)ctiles, (int)pgroups, out_dev, first_out_dev);
    CTPVAE_LAUNCH_CHECK("convt_fwd_kernel");
    return CTPVAE_OK;
}

int ctpvae_convt_bwd_weight_f32(const float *x_dev, const float *g_dev, const unsigned char *first_dev, int N, int Cin, int H, int W, int C,
                                int k, int s, int pad, int opad, void *workspace_dev, float *gw_out_dev, float *gb_out_dev,
                                ctpvae_stream_t stream)
{
    CTPVAE_REQUIRE(x_dev && g_dev && first_dev && workspace_dev && gw_out_dev && gb_out_dev, "convt_bwd_weight: null pointer");
    ConvtGeom gm;
    if (int rc = convt_check("convt_bwd_weight", N, Cin, H, W, C, k, s, pad, opad, &gm)) return rc;
    int chunks, chunks_o;
    CTPVAE_REQUIRE(convt_wgrad_floats(gm, &chunks, &chunks_o) >= 0, "convt_bwd_weight: chunks * Cin * 2C * k * k + output chunks * 2C must fit "
                   "31 bits (chunks=%d and %d Cin=%d C=%d k=%d)", chunks, chunks_o, Cin, C, k);
    const long long ctiles = ceil_div(C, 32), citiles = ceil_div(Cin, 32);
    const long long wwaves = chunks * ctiles * citiles * k * k, bwaves = chunks_o * ctiles;
    const long long wblocks = ceil_div(wwaves, 4), blocks = wblocks + ceil_div(bwaves, 4);
    // blocks * 4, the kernel's wave index, must fit too; wwaves and bwaves are below it
    if (int rc = conv_check_blocks("convt_bwd_weight", blocks, INT_MAX / 4)) return rc;
    const unsigned totalw = (unsigned)Cin * 2u * (unsigned)C * (unsigned)(k * k);
    float *part = (float *)workspace_dev, *partb = part + (size_t)chunks * totalw;
    hipLaunchKernelGGL(convt_wgrad_kernel, dim3((unsigned)blocks), dim3(kConvThreads), 0, (hipStream_t)stream, x_dev, g_dev, first_dev, gm,
                       (int)ctiles, (int)citiles, (int)wwaves, (int)wblocks, (int)bwaves, N * gm.HW, N * gm.P, part, partb);
    CTPVAE_LAUNCH_CHECK("convt_wgrad_kernel");
    hipLaunchKernelGGL(convt_wgrad_finish_kernel, dim3((totalw + 2u * C + kConvThreads - 1) / kConvThreads), dim3(kConvThreads), 0,
                       (hipStream_t)stream, (const float *)part, (const float *)partb, chunks, chunks_o, totalw, 2u * (unsigned)C, gw_out_dev,
                       gb_out_dev);
    CTPVAE_LAUNCH_CHECK("convt_wgrad_finish_kernel");
    return CTPVAE_OK;
}

int ctpvae_convt_bwd_input_f32(const float *g_dev, const unsigned char *first_dev, const float *w_dev, int N, int Cin, int H, int W, int C,
                               int k, int s, int pad, int opad, float *gx_out_dev, ctpvae_stream_t stream)
{
    CTPVAE_REQUIRE(g_dev && first_dev && w_dev && gx_out_dev, "convt_bwd_input: null pointer");
    ConvtGeom gm;
    if (int rc = convt_check("convt_bwd_input", N, Cin, H, W, C, k, s, pad, opad, &gm)) return rc;
    const long long citiles = ceil_div(Cin, 32), pgroups = ceil_div(gm.HW, 128), blocks = (long long)N * citiles * pgroups;
    if (int rc = conv_check_blocks("convt_bwd_input", blocks)) return rc;
    hipLaunchKernelGGL(convt_dgrad_kernel, dim3((unsigned)blocks), dim3(kConvThreads), 0, (hipStream_t)stream, g_dev, first_dev, w_dev, gm,
                       (int)citiles, (int)pgroups, gx_out_dev);
    CTPVAE_LAUNCH_CHECK("convt_dgrad_kernel");
    return CTPVAE_OK;
}

}  // extern "C"
