// conv_tile.h -- what conv.hip and conv_transpose.hip share: the workgroup's size, the chunk rule's length, the depth of the k loop's
// prefetch and the accumulator tile of v_mfma_f32_32x32x2_f32 (conv.hip's header states the instruction's lane maps).
#pragma once

namespace ctpvae {

constexpr int kConvThreads = 256;      // four waves
constexpr int kConvChunk = 1024;       // the chunk rule of the weight gradient
constexpr int kConvMaxK = 8;
constexpr int kConvDepth = 4;          // steps of the k loop whose loads are issued before their MFMAs; no effect on any result

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the row of the 32 x 32 tile that register `reg` of a lane in half `half` (lane >> 5) holds; the column is lane & 31
__device__ __forceinline__ int tile_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

}  // namespace ctpvae
