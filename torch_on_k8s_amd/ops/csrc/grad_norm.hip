// Global gradient L2 norm + clip coefficient on flat bf16 buckets (MI355X).
//
// Two kernels, both capturable into a hipGraph (no allocation, no sync):
//
//   sumsq_kernel     one streaming pass over a bucket. Each block writes ONE
//                    fp32 partial to its own slot of a caller-owned
//                    workspace with a plain store.
//   finalize_kernel  one block sums every partial of every bucket in a fixed
//                    order and writes {norm, gscale} as two device floats
//                    that the AdamW kernel reads.
//
// No float atomics anywhere: the order of every addition is fixed by the
// launch geometry alone, so the training step stays bitwise repeatable. The
// kernel boundary between the two is what makes the partials (written by
// blocks on all XCDs) visible to the single finalize block.
#include "common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int UNROLL = 4;         // independent 16 B loads + accumulators
constexpr int MAX_BLOCKS = 2048;  // same grid cap as adamw.hip
constexpr int FIN_BLOCK = 1024;

// a bf16 has 8 significant bits, so f*f is exact in fp32; the only rounding
// is in the adds
DEVINL float sumsq8(const bf16x8 v, float acc) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float f = bfbits2f(v.h[j]);
    acc = fmaf(f, f, acc);
  }
  return acc;
}

__global__ void __launch_bounds__(BLOCK)
sumsq_kernel(const bf16x8* __restrict__ g, long nvec,
             float* __restrict__ partials) {
  __shared__ float wsum[BLOCK / WAVE];
  const long stride = (long)gridDim.x * BLOCK;
  long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  float acc[UNROLL] = {0.f, 0.f, 0.f, 0.f};
  // full sweeps: UNROLL loads issued back to back, one accumulator each
  for (; i + (UNROLL - 1) * stride < nvec; i += UNROLL * stride) {
    bf16x8 v[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) v[u] = g[i + u * stride];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) acc[u] = sumsq8(v[u], acc[u]);
  }
  // ragged last sweep (fewer than UNROLL vectors left for this thread)
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    const long idx = i + u * stride;
    if (idx < nvec) acc[u] = sumsq8(g[idx], acc[u]);
  }
  float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  s = wave_reduce_sum(s);
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  if (lane == 0) wsum[wid] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = wsum[0];
#pragma unroll
    for (int w = 1; w < BLOCK / WAVE; ++w) t += wsum[w];
    partials[blockIdx.x] = t;  // a block with no work writes 0
  }
}

__global__ void __launch_bounds__(FIN_BLOCK)
finalize_kernel(const float* __restrict__ partials, long count,
                float inv_count, float clip, float* __restrict__ out) {
  __shared__ float scratch[FIN_BLOCK / WAVE];
  float s = 0.f;
#pragma unroll 8
  for (long i = threadIdx.x; i < count; i += FIN_BLOCK) s += partials[i];
  const float total = block_reduce_sum(s, scratch);
  if (threadIdx.x == 0) {
    const float norm = sqrtf(total) * inv_count;
    float coef = 1.f;
    if (clip > 0.f) {
      coef = clip / (norm + 1e-6f);
      // not fminf: a NaN norm must poison the step exactly as the host
      // clamp does, not silently turn into "no clip"
      if (coef > 1.f) coef = 1.f;
    }
    out[0] = norm;
    out[1] = inv_count * coef;
  }
}

}  // namespace

extern "C" {

int tok_grad_sumsq_max_blocks() { return MAX_BLOCKS; }

// Number of partial slots (= blocks) a bucket of n elements uses.
int tok_grad_sumsq_blocks(long n) {
  long b = (n / 8 + BLOCK - 1) / BLOCK;
  if (b > MAX_BLOCKS) b = MAX_BLOCKS;
  if (b < 1) b = 1;
  return (int)b;
}

// g: flat contiguous bf16, n a multiple of 8. Writes exactly `nblocks`
// floats to `partials` (block b -> partials[b]); nblocks in [1, MAX_BLOCKS].
hipError_t tok_grad_sumsq(const void* g, long n, float* partials, int nblocks,
                          hipStream_t stream) {
  if (nblocks < 1 || nblocks > MAX_BLOCKS || n % 8 != 0)
    return hipErrorInvalidValue;
  sumsq_kernel<<<nblocks, BLOCK, 0, stream>>>((const bf16x8*)g, n / 8,
                                              partials);
  return hipGetLastError();
}

// out[0] = sqrt(sum(partials)) * inv_count
// out[1] = inv_count * min(1, clip / (out[0] + 1e-6))   (clip <= 0: no clip)
hipError_t tok_grad_norm_finalize(const float* partials, long count,
                                  float inv_count, float clip, float* out,
                                  hipStream_t stream) {
  finalize_kernel<<<1, FIN_BLOCK, 0, stream>>>(partials, count, inv_count,
                                               clip, out);
  return hipGetLastError();
}
}
