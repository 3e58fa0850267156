// FP8 weight-only linear for ragged decode on MI355X (gfx950): a skinny-M
// MFMA GEMM that streams e4m3 weights, and the dequantizer the prefill uses.
//
//   y[M,N] = x[M,K] . (float(code[N,K]) * wscale[N])^T
//   x, y bf16; code OCP e4m3 bytes in the nn.Linear layout ([N,K], K
//   contiguous); wscale one fp32 per output channel.
//   Contract: 1 <= M <= 64, K % 128 == 0, N % 16 == 0.
//
//   linear_w8_kernel<MT>   grid (ceil(N/64), num_splits), 256 threads
//     MT = ceil(M/16) token tiles (1..4). Wave w of block (bx, z) owns output
//     channels n0 + 16w .. +15 (n0 = 64 bx) over split z's K range: no two
//     waves share an output and nothing is merged inside a block. A wave whose
//     channels start at or past N (the last block when N % 64 != 0) streams
//     row N - 1 instead and stores nothing: every wave then issues the same
//     loads, does its share of the x staging and takes part in the barriers.
//     Split z owns a contiguous run of the K/128 steps: with q = steps / S and
//     r = steps % S, split z starts at z q + min(z, r) and has q + (z < r)
//     steps. A split with no steps writes zero partials and reads nothing.
//
// Products, mfma_f32_16x16x32_bf16, four per 128-step. A operand: lane
// (i = lane & 15, g = lane >> 4) holds row i, k-slots 8g..8g+7; B operand:
// column i, the same k-slots; C: column i, rows 4g..4g+3.
//   W is A. Lane (i, g) holds channel n0 + 16w + i. The stream goes global ->
//   VGPR, never through LDS (a wave reads its rows exactly once): two 16-byte
//   loads per lane per step, load j covering bytes 64j + 16g .. +15 of the
//   row's 128-byte step, so the four g-lanes of a row cover one contiguous
//   64-byte piece per load instruction. The two halves h of a load feed two
//   MFMAs. K order inside a step: k-slot e of lane (i, g) in MFMA 2j + h is
//       k = 64 j + 16 g + 8 h + e,
//   and the x fragments use the same map. Codes are widened in registers:
//   v_cvt_pk_f32_fp8 (two codes) and one v_cvt_pk_bf16_f32 per pair; every
//   e4m3 value is a bf16 value, both steps are exact. 16 VALU instructions
//   per 16 bytes, paid once per 16 channels x 32 k whatever M is: each widened
//   fragment feeds one MFMA per token tile.
//   x is B. Column i of tile mt is token 16 mt + i. The accumulators are four
//   VGPRs per token tile: lane (i, g) ends with token 16 mt + i, channels
//   n0 + 16w + 4g + 0..3.
//
// W pipeline. Step t's two loads are issued two steps ahead (three register
// sets, the loop is unrolled by three so the sets have fixed names): when
// W(t) is first consumed W(t+1) and W(t+2) follow it, so four 16-byte loads
// per lane are in flight before the first is consumed.
//
// x staging. The block's x slice for one step, [16 MT tokens][128 k] bf16 =
// MT * 4096 bytes, goes global -> LDS by 16-byte DMA (global_load_lds_dwordx4,
// the inline-asm form: the builtin forces vmcnt(0)); two buffers. Wave w's
// DMA instruction q writes the 1024 bytes (four rows) at (4q + w) * 1024:
// lane l lands at row 4(4q + w) + (l >> 4), slot l & 15. The source row is
// min(row, M - 1): a row past M is never read from memory, and a pad column's
// result is never stored. Per step, in this order:
//     s_waitcnt vmcnt(2)        x(t) landed in this wave; W(t+1)'s two loads,
//                               issued after it, may stay in flight
//                               (vmcnt(0) where the step before loaded no W)
//     barrier                   x(t) landed in every wave, and every wave is
//                               done reading the other buffer (step t-1)
//     widen W(t)                the compiler's own vmcnt(2) for W(t), exact
//     DMA x(t+1), load W(t+2)   in that order, pinned by sched_barrier
//     ds_read x(t), MFMAs
// One barrier per step. The DMA is invisible to the compiler's vmcnt
// counting; it only ever makes a compiler-placed wait stronger, and the order
// above keeps the DMA out of every window the compiler waits on.
//
// LDS image and swizzle. A tile row is 256 bytes = sixteen 16-byte chunks =
// exactly one bank row (bank = (addr / 4) % 64, the rule of attn_extend.hip;
// a b128 read is served 16 lanes at a time). The fragment read of MFMA 2j + h
// takes chunk c = 8j + 2g + h of row i: the 16 lanes served together are rows
// 0..15 of ONE chunk, which unswizzled is one slot 16 times. Chunk c of row r
// is stored at slot c ^ (r & 15): for fixed c the slots of rows 0..15 are
// c ^ 0 .. c ^ 15, a bijection of 0..15, so the 16 lanes hit 16 different
// slots = all 64 banks once: conflict-free. The DMA writes LDS linearly, so
// the XOR is applied to the global source chunk and again to the read.
//
// Epilogue. acc * wscale[n] is one fp32 multiply, applied BEFORE the split
// fold at every split count. num_splits == 1: round once to bf16, one 8-byte
// store of y[token][n .. n+3] per lane and tile. num_splits > 1: the scaled
// fp32 partials go to ws[split][M][N] (one 16-byte store) and
// linear_w8_combine_kernel adds them in split order, 0 first, applies nothing
// else and rounds once. No atomics, every sum in a fixed order; the grid
// depends on shapes alone: capturable, bitwise repeatable, and a token's row
// does not depend on its batch slot (a column of B only meets its own
// accumulator column).
// fp32 budget (tests/test_linear_w8_gpu.py counts k from this): one MFMA
// chain over the split's products, at most 128 * ceil(steps / S) terms, one
// rounding per term; the scale multiply; S - 1 adds in the combine.
//
//   w8_dequant_kernel   grid-stride, 256 threads
//     out[N,K] bf16 = bf16(float(code) * wscale[n]): one fp32 product, one
//     round to nearest even; 16 codes per thread (one 16-byte load, two
//     16-byte stores). Serves M > 64 (the prefill): dequantize, then the
//     library GEMM of the bf16 path.
//
// Resources (hipcc -O3 --offload-arch=gfx950,
// -Rpass-analysis=kernel-resource-usage; scratch is 0 B everywhere):
//   kernel                     VGPR  AGPR  SGPR  LDS B  waves/SIMD
//   linear_w8_kernel<1>          55     4    39   8192  8
//   linear_w8_kernel<2>          56     8    39  16384  8
//   linear_w8_kernel<3>          58    12    39  24576  6
//   linear_w8_kernel<4>          59    16    39  32768  5
//   linear_w8_combine_kernel     14     0    39      0  8
//   w8_dequant_kernel            27     0    39      0  8
// ISA read (--save-temps): inside the loop every s_waitcnt vmcnt is (2) or
// (3); the only vmcnt(0) are the second tail step's and the one after the
// loop, and none sits next to a global_load.
#include "common.h"

#include <type_traits>

namespace {

#if defined(__HIP_DEVICE_COMPILE__)
#define W8_KERNEL __global__ __attribute__((target("no-packed-fp32-ops")))
#else
#define W8_KERNEL __global__
#endif

using bf16x8v = __attribute__((ext_vector_type(8))) __bf16;
using bf16x2v = __attribute__((ext_vector_type(2))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;

constexpr int W8_NTH = 256;
constexpr int W8_BN = 64;          // output channels per block
constexpr int W8_KS = 128;         // k per step
constexpr int W8_ROW = W8_KS * 2;  // bytes of one x tile row

// 16 bytes per lane, global -> LDS: lane i's bytes land at lds_dst + 16 i.
DEVINL void w8_glds16(uint32_t voff, const void* sbase, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_dst)
      : "memory");
}

DEVINL void w8_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

DEVINL uint32_t w8_pack(float lo, float hi) {
  const f32x2 f = {lo, hi};
  union { bf16x2v b; uint32_t u; } c;
  c.b = __builtin_convertvector(f, bf16x2v);
  return c.u;
}

// 8 e4m3 codes (two dwords) -> 8 bf16, byte j = element j; exact
DEVINL bf16x8v w8_widen(uint32_t lo, uint32_t hi) {
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false);
  const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
  const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false);
  const f32x2 d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
  union { uint32_t w[4]; bf16x8v f; } r;
  r.w[0] = w8_pack(a[0], a[1]);
  r.w[1] = w8_pack(b[0], b[1]);
  r.w[2] = w8_pack(c[0], c[1]);
  r.w[3] = w8_pack(d[0], d[1]);
  return r.f;
}

template <int MT>
W8_KERNEL __launch_bounds__(W8_NTH) void linear_w8_kernel(
    const bf16_t* __restrict__ x, const uint8_t* code,
    const float* __restrict__ wscale, bf16_t* __restrict__ y,
    float* __restrict__ ws, int M, int N, int K) {
  constexpr int TILE = MT * 16 * W8_ROW;  // one x buffer
  __shared__ __attribute__((aligned(1024))) char smem[2 * TILE];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int z = blockIdx.y, S = gridDim.y;
  const int nw = blockIdx.x * W8_BN + wid * 16;  // the wave's first channel
  const bool live = nw < N;                      // wave-uniform

  const int steps = K / W8_KS;
  const int sq = steps / S, sr = steps % S;
  const int s0 = z * sq + min(z, sr);
  const int ns = sq + (z < sr ? 1 : 0);

  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (ns > 0) {  // block-uniform
    // ---- DMA geometry: instruction q of this wave, lane l ----
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem +
        wid * 1024);
    uint32_t d_off[MT];
#pragma unroll
    for (int q = 0; q < MT; ++q) {
      const int r = 4 * (4 * q + wid) + lg;
      d_off[q] = (uint32_t)min(r, M - 1) * (uint32_t)K * 2 +
                 16 * (li ^ (r & 15));
    }
    const char* xs = reinterpret_cast<const char*>(x) + (long)s0 * W8_ROW;

    // ---- fragment read offsets within a tile row block ----
    uint32_t b_off[4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
      b_off[m] = li * W8_ROW + 16 * ((8 * (m >> 1) + 2 * lg + (m & 1)) ^ li);

    // ---- the lane's W row (a wave with no channels streams row N - 1) ----
    const uint8_t* wrow =
        code + (long)min(nw + li, N - 1) * K + (long)s0 * W8_KS + 16 * lg;
    // a step past the split's end loads these 64 bytes instead (one cache
    // line per instruction, never consumed): the count of loads in flight
    // stays the same at every step, which is what keeps vmcnt(2) exact
    const uint8_t* wpad = code + 16 * lg;

    uint4 wr[3][2];
    // prologue, in the loop's order: W(0), x(0), W(1)
    wr[0][0] = *reinterpret_cast<const uint4*>(wrow);
    wr[0][1] = *reinterpret_cast<const uint4*>(wrow + 64);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < MT; ++q) w8_glds16(d_off[q], xs, lds0 + q * 4096);
    __builtin_amdgcn_sched_barrier(0);
    {
      const uint8_t* p = ns > 1 ? wrow + W8_KS : wpad;
      wr[1][0] = *reinterpret_cast<const uint4*>(p);
      wr[1][1] = *reinterpret_cast<const uint4*>(p + 64);
      asm volatile("" ::: "memory");
    }
    __builtin_amdgcn_sched_barrier(0);

    // One step, a single basic block: u names the register set of W(t).
    // tail 0 is a step of the loop; 1 and 2 are the first and second step
    // after it, which load no W (nothing would consume it), so the second
    // finds only x(t) in flight. `code` is not __restrict__ on purpose: the
    // "memory" asm statements then fence the W loads, and the counts below
    // are the counts in the ISA.
    auto step = [&](auto uc, auto tc, int t) __attribute__((always_inline)) {
      constexpr int u = decltype(uc)::value;
      constexpr int tail = decltype(tc)::value;
      // x(t) landed in this wave; W(t+1)'s two loads may stay in flight
      if constexpr (tail == 2)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      w8_barrier();

      bf16x8v a[4];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        a[2 * j] = w8_widen(wr[u][j].x, wr[u][j].y);
        a[2 * j + 1] = w8_widen(wr[u][j].z, wr[u][j].w);
      }
      // volatile asm keeps its order: the widening (and the compiler's wait
      // for W(t)) stays above the DMA, where exactly W(t+1) is in flight
      asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]));
      __builtin_amdgcn_sched_barrier(0);
      {  // the tile after the last is the last again; nobody reads it
        const char* src = xs + (long)min(t + 1, ns - 1) * W8_ROW;
        const uint32_t dst = lds0 + ((t + 1) & 1) * TILE;
#pragma unroll
        for (int q = 0; q < MT; ++q) w8_glds16(d_off[q], src, dst + q * 4096);
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (tail == 0) {
        const uint8_t* p = t + 2 < ns ? wrow + (long)(t + 2) * W8_KS : wpad;
        wr[(u + 2) % 3][0] = *reinterpret_cast<const uint4*>(p);
        wr[(u + 2) % 3][1] = *reinterpret_cast<const uint4*>(p + 64);
        asm volatile("" ::: "memory");
      }
      __builtin_amdgcn_sched_barrier(0);
      const char* xt = smem + (t & 1) * TILE;
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          union { uint4 u; bf16x8v f; } b;
          b.u = *reinterpret_cast<const uint4*>(xt + mt * 16 * W8_ROW +
                                                b_off[m]);
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m], b.f, acc[mt],
                                                            0, 0, 0);
        }
      __builtin_amdgcn_sched_barrier(0);
    };
    using C0 = std::integral_constant<int, 0>;
    using C1 = std::integral_constant<int, 1>;
    using C2 = std::integral_constant<int, 2>;

    int t = 0;
    for (; t + 3 <= ns; t += 3) {
      step(C0{}, C0{}, t);
      step(C1{}, C0{}, t + 1);
      step(C2{}, C0{}, t + 2);
    }
    if (t < ns) step(C0{}, C1{}, t);
    if (t + 1 < ns) step(C1{}, C2{}, t + 1);
    // the last step's DMA must not land in an LDS that is no longer ours
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }

  if (!live) return;
  const int n = nw + 4 * lg;  // this lane's four channels
  float sc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) sc[j] = wscale[n + j];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int tok = 16 * mt + li;
    if (tok >= M) continue;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = acc[mt][j] * sc[j];
    if (S == 1) {
      *reinterpret_cast<uint2*>(y + (long)tok * N + n) =
          make_uint2(w8_pack(v[0], v[1]), w8_pack(v[2], v[3]));
    } else {
      *reinterpret_cast<f32x4v*>(ws + ((long)z * M + tok) * N + n) =
          f32x4v{{v[0], v[1], v[2], v[3]}};
    }
  }
}

// y = bf16(sum over splits, in split order, of ws[split][M*N]); 4 per thread
W8_KERNEL void linear_w8_combine_kernel(const f32x4v* __restrict__ ws,
                                        uint2* __restrict__ y, long nvec,
                                        int S) {
  for (long i = (long)blockIdx.x * W8_NTH + threadIdx.x; i < nvec;
       i += (long)gridDim.x * W8_NTH) {
    f32x4v s = ws[i];
    for (int z = 1; z < S; ++z) {
      const f32x4v p = ws[z * nvec + i];
#pragma unroll
      for (int j = 0; j < 4; ++j) s.v[j] += p.v[j];
    }
    y[i] = make_uint2(w8_pack(s.v[0], s.v[1]), w8_pack(s.v[2], s.v[3]));
  }
}

// 16 codes of one row per thread; kv = K / 16 vectors per row
W8_KERNEL void w8_dequant_kernel(const uint4* __restrict__ code,
                                 const float* __restrict__ wscale,
                                 uint4* __restrict__ out, long nvec, int kv) {
  for (long i = (long)blockIdx.x * W8_NTH + threadIdx.x; i < nvec;
       i += (long)gridDim.x * W8_NTH) {
    const float s = wscale[i / kv];
    const uint4 c = code[i];
    const uint32_t d[4] = {c.x, c.y, c.z, c.w};
    uint32_t o[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)d[j], false);
      const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)d[j], true);
      o[2 * j] = w8_pack(lo[0] * s, lo[1] * s);
      o[2 * j + 1] = w8_pack(hi[0] * s, hi[1] * s);
    }
    out[2 * i] = make_uint4(o[0], o[1], o[2], o[3]);
    out[2 * i + 1] = make_uint4(o[4], o[5], o[6], o[7]);
  }
}

int w8_grid(long nwork) {
  long grid = (nwork + W8_NTH - 1) / W8_NTH;
  if (grid > 8192) grid = 8192;
  if (grid < 1) grid = 1;
  return (int)grid;
}

template <int MT>
void launch_w8(const void* x, const void* code, const float* wscale, void* y,
               float* ws, int M, int N, int K, int num_splits,
               hipStream_t stream) {
  dim3 grid((N + W8_BN - 1) / W8_BN, num_splits);
  linear_w8_kernel<MT><<<grid, W8_NTH, 0, stream>>>(
      (const bf16_t*)x, (const uint8_t*)code, wscale, (bf16_t*)y, ws, M, N, K);
}

}  // namespace

extern "C" {

// linear_w8_combine_kernel over nvec 4-float groups: y = bf16(the sum of the
// num_splits fp32 partial images in ws, in split order). linear_w4.hip folds
// its splits through it as well.
hipError_t tok_split_combine(const float* ws, void* y, long nvec,
                             int num_splits, hipStream_t stream) {
  linear_w8_combine_kernel<<<w8_grid(nvec), W8_NTH, 0, stream>>>(
      (const f32x4v*)ws, (uint2*)y, nvec, num_splits);
  return hipGetLastError();
}

// ws: fp32, num_splits*M*N elements; unused when num_splits == 1.
hipError_t tok_linear_w8(const void* x, const void* code, const float* wscale,
                         void* y, float* ws, int M, int N, int K,
                         int num_splits, hipStream_t stream) {
  if (M < 1 || M > 64 || K < W8_KS || K % W8_KS != 0 || N < 16 ||
      N % 16 != 0 || num_splits < 1 || num_splits > 65535 ||
      (num_splits > 1 && ws == nullptr))
    return hipErrorInvalidValue;
  switch ((M + 15) / 16) {
    case 1: launch_w8<1>(x, code, wscale, y, ws, M, N, K, num_splits, stream); break;
    case 2: launch_w8<2>(x, code, wscale, y, ws, M, N, K, num_splits, stream); break;
    case 3: launch_w8<3>(x, code, wscale, y, ws, M, N, K, num_splits, stream); break;
    default: launch_w8<4>(x, code, wscale, y, ws, M, N, K, num_splits, stream); break;
  }
  HIP_CHECK(hipGetLastError());
  if (num_splits > 1)
    HIP_CHECK(tok_split_combine(ws, y, (long)M * N / 4, num_splits, stream));
  return hipSuccess;
}

hipError_t tok_w8_dequant(const void* code, const float* wscale, void* out,
                          long N, int K, hipStream_t stream) {
  if (N < 1 || K < 16 || K % 16 != 0) return hipErrorInvalidValue;
  const long nvec = N * (K / 16);
  w8_dequant_kernel<<<w8_grid(nvec), W8_NTH, 0, stream>>>(
      (const uint4*)code, wscale, (uint4*)out, nvec, K / 16);
  return hipGetLastError();
}
}
