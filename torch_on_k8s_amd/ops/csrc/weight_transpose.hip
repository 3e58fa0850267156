// 2-D transpose of a bf16 matrix: out[C, R] = in[R, C]^T, both row-major.
//
// Why: dx = dy . W is an NN product for the GEMM library, the layout it has
// no tuned kernel for. With Wt = W^T as a row-major [K, N] tensor the same
// product is the TN call of the forward pass, dx = F.linear(dy, Wt). This
// memory-bound kernel makes Wt from the live weight right before the GEMM.
//
// It moves 16-bit patterns, never numbers: NaN payloads, -0 and subnormals
// come out as they went in.
//
// Structure per 64x64 tile (one 256-thread block), as transpose_head_kernel:
//   16-byte global loads (8 lanes cover 128 B of one input row)
//   -> swizzled row-major LDS tile (conflict-free b128 writes)
//   -> per-thread column gather (8 x u16 LDS reads)
//   -> 16-byte global stores (8 lanes cover 128 B of one output row)
// R and C are multiples of 8, so a 16-byte vector is wholly inside the
// matrix or wholly outside; partial tiles are guarded per vector in both
// directions.
#include "common.h"

namespace {

constexpr int WT_T = 64;       // tile side
constexpr int WT_NT = 256;     // threads per block

DEVINL int wt_swz(int row, int byte_in_row) {
  return byte_in_row ^ ((row & 7) << 4);
}

__global__ __launch_bounds__(WT_NT) void weight_transpose_kernel(
    const uint16_t* __restrict__ in,   // [R, C]
    uint16_t* __restrict__ out,        // [C, R]
    long R, long C) {
  __shared__ __attribute__((aligned(16))) char lds[WT_T * WT_T * 2];
  const long c0 = (long)blockIdx.x * WT_T;
  const long r0 = (long)blockIdx.y * WT_T;

  // load 64 x 64 (r x c), two passes of 32 rows
#pragma unroll
  for (int p = 0; p < WT_T * (WT_T / 8) / WT_NT; ++p) {
    const int vi = threadIdx.x + p * WT_NT;
    const int row = vi / 8, cv = vi % 8;
    uint4 val = {0, 0, 0, 0};
    if (r0 + row < R && c0 + cv * 8 < C)
      val = *(const uint4*)(in + (r0 + row) * C + c0 + cv * 8);
    *(uint4*)(lds + row * 128 + wt_swz(row, cv * 16)) = val;
  }
  __syncthreads();

  // emit 64 x 64 (c x r): thread u covers out row c0+(u>>3), r chunk (u&7)*8
#pragma unroll
  for (int p = 0; p < WT_T * (WT_T / 8) / WT_NT; ++p) {
    const int u = threadIdx.x + p * WT_NT;
    const int cr = u >> 3;              // c-local (two passes: 0..31, 32..63)
    const int rc = (u & 7) * 8;         // r-local chunk start
    uint16_t vals[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int r = rc + j;
      vals[j] = *(const uint16_t*)(lds + r * 128 + wt_swz(r, cr * 2));
    }
    if (c0 + cr < C && r0 + rc < R)
      *(uint4*)(out + (c0 + cr) * R + r0 + rc) = *(const uint4*)vals;
  }
}

}  // namespace

extern "C" {

// One launch on `stream`; allocates nothing and does not sync. The caller
// guarantees that in and out do not overlap.
hipError_t tok_transpose_2d(const void* in, void* out, long R, long C,
                            hipStream_t stream) {
  if (R <= 0 || C <= 0 || R % 8 != 0 || C % 8 != 0)
    return hipErrorInvalidValue;
  if (((uintptr_t)in | (uintptr_t)out) % 16 != 0) return hipErrorInvalidValue;
  const long gx = (C + WT_T - 1) / WT_T, gy = (R + WT_T - 1) / WT_T;
  if (gx > 2147483647L || gy > 65535L) return hipErrorInvalidValue;
  dim3 grid((unsigned)gx, (unsigned)gy, 1);
  weight_transpose_kernel<<<grid, WT_NT, 0, stream>>>(
      (const uint16_t*)in, (uint16_t*)out, R, C);
  return hipGetLastError();
}
}
