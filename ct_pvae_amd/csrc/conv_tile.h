// conv_tile.h -- what conv.hip and conv_transpose.hip share: the workgroup's size, the chunk rule's length and range, the depth of the
// k loop's prefetch, the accumulator tile of v_mfma_f32_32x32x2_f32 with its lane maps, the steps and stores on that tile that both
// files take (zeroing, the selected-pair step, the maxout store, the ascending sum of the chunks' partials), the branch-free masked
// load, and the host-side requirements that both geometries make.  The index walks -- which element a lane loads at which step --
// differ and stay in their files.
//
// The matrix instruction.  D = A * B + C with A [32][2], B [2][32], C/D [32][32]: lane l holds A[l & 31][l >> 5] and B[l >> 5][l & 31];
// register g of lane l holds D[(g & 3) + 8 * (g >> 2) + 4 * (l >> 5)][l & 31].  Per element it is the chain
// fmaf(a1, b1, fmaf(a0, b0, c)) -- k ascending, one rounding per product -- so a loop of them over ascending k is one fmaf chain.
// (tests/test_gpu_conv.py checks the lane maps with small asymmetric integers and the chain by bits against the twin: on the MI355X
// the instruction delivers exactly these bits, so no kernel of either file has an explicit-fmaf VALU path.)
// Channels lie on the ROWS (A = weights or cotangents), pixels or taps on the COLUMNS (B), so a register's 32 lanes store 32
// consecutive floats.  A wave computes TWO tiles that share B: rows c0 .. c0 + 31 of the first channel half and the SAME channels of
// the second half, so the maxout's two operands meet in one register slot of one lane.
// An operand outside its range (a row past C or Cin, a column past the pixels, a k past the sum's length) is fed as +0.
#pragma once

#include <climits>

#include "common.h"

namespace ctpvae {

constexpr int kConvThreads = 256;      // four waves
constexpr int kConvChunk = 1024;       // the chunk rule of the weight gradient
constexpr int kConvMaxK = 8;
constexpr int kConvDepth = 4;          // steps of the k loop whose loads are issued before their MFMAs; no effect on any result

typedef float f32x16 __attribute__((ext_vector_type(16)));

// a thread's place: its wave of the workgroup, its row of A / column of B (lane & 31) and its k of the instruction's two (lane >> 5)
struct TileLane {
    int wv, j, half;
};

__device__ __forceinline__ TileLane tile_lane()
{
    const int lane = threadIdx.x & 63;
    return TileLane{(int)(threadIdx.x >> 6), lane & 31, lane >> 5};
}

// the row of the 32 x 32 tile that register `reg` of a lane in half `half` (lane >> 5) holds; the column is lane & 31
__device__ __forceinline__ int tile_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

__device__ __forceinline__ void tile_zero(f32x16 &acc)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
}

// one step of the backward's tile pair: the cotangent g enters the tile of the half that the maxout took and +0 the other's, by
// SELECTION (first ? g : +0 and first ? +0 : g), over the shared column operand b
__device__ __forceinline__ void tile_mfma_selected(f32x16 &accA, f32x16 &accB, bool first, float g, float b)
{
    accA = __builtin_amdgcn_mfma_f32_32x32x2f32(first ? g : 0.0f, b, accA, 0, 0, 0);
    accB = __builtin_amdgcn_mfma_f32_32x32x2f32(first ? 0.0f : g, b, accB, 0, 0, 0);
}

// the maxout of a wave's two tiles, stored: rows ct * 32 + tile_row(g, half) < C of object n at pixel pix of P; first = a >= b (a tie
// takes the first half, a NaN on either side the second), out = first ? a : b, one `first` byte (0 or 1) per element
__device__ __forceinline__ void tile_store_maxout(const f32x16 &accA, const f32x16 &accB, int ct, int half, int n, int C, int P, int pix,
                                                  float *__restrict__ out, unsigned char *__restrict__ first_out)
{
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const int cr = ct * 32 + tile_row(g, half);
        if (cr < C) {
            const float a = accA[g], b = accB[g];
            const bool first = a >= b;
            const size_t o = ((size_t)n * C + cr) * P + pix;
            out[o] = first ? a : b;
            first_out[o] = first ? 1 : 0;
        }
    }
}

// CHUNK RULE: the `total` terms of a sum are cut into chunks of kConvChunk consecutive ones (the last one shorter), a function of
// `total` alone; chunk `chunk` holds [m_begin, m_end)
__device__ __forceinline__ void chunk_range(int chunk, int total, int &m_begin, int &m_end)
{
    m_begin = chunk * kConvChunk;
    m_end = total - m_begin < kConvChunk ? total : m_begin + kConvChunk;
}

// the chunks' partials of element e (chunk jc's at part[jc * stride + e]) in ascending order, in fp32, starting from the first
__device__ __forceinline__ float chunk_sum(const float *__restrict__ part, int chunks, size_t stride, size_t e)
{
    float acc = part[e];
    for (int jc = 1; jc < chunks; ++jc) acc = acc + part[jc * stride + e];
    return acc;
}

// p[i] where ok, +0 elsewhere, with no branch: the load is always issued (from element 0 where !ok, which every operand has) and its
// BITS are masked, which is a selection (a NaN or an infinity that is not wanted leaves no trace).  So a group's loads stay in
// flight together; written as a select of the loaded value the compiler puts each load behind a branch of its own and waits there.
__device__ __forceinline__ float load_or_zero(const float *__restrict__ p, bool ok, size_t i)
{
    return __uint_as_float(__float_as_uint(p[ok ? i : 0]) & (ok ? 0xffffffffu : 0u));
}

__device__ __forceinline__ unsigned char load_or_zero(const unsigned char *__restrict__ p, bool ok, size_t i)
{
    return (unsigned char)(p[ok ? i : 0] & (ok ? 0xffu : 0u));
}

// ---- host side: what both geometries require, `what` naming the entry point ----

inline long long ceil_div(long long n, int per) { return (n + per - 1) / per; }

inline int conv_check_common(const char *what, int N, int Cin, int H, int W, int C, int k, int s)
{
    CTPVAE_REQUIRE(N >= 1 && Cin >= 1 && H >= 1 && W >= 1 && C >= 1, "%s: extents must be at least 1 (N=%d Cin=%d H=%d W=%d C=%d)", what, N,
                   Cin, H, W, C);
    CTPVAE_REQUIRE(k >= 1 && k <= kConvMaxK, "%s: the kernel size must be in 1 .. %d (got %d)", what, kConvMaxK, k);
    CTPVAE_REQUIRE(s >= 1 && s <= k, "%s: the stride must be in 1 .. k (got s=%d k=%d)", what, s, k);
    return CTPVAE_OK;
}

// a launch's workgroups must fit 31 bits (`limit` lower where the kernel multiplies its workgroup index)
inline int conv_check_blocks(const char *what, long long blocks, long long limit = INT_MAX)
{
    CTPVAE_REQUIRE(blocks <= limit, "%s: %lld workgroups do not fit 31 bits", what, blocks);
    return CTPVAE_OK;
}

}  // namespace ctpvae
