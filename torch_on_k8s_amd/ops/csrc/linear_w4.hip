// MXFP4 weight-only linear for ragged decode on MI355X (gfx950): a skinny-M
// MFMA GEMM that streams e2m1 weight codes with one e8m0 scale per 32
// elements, and the dequantizer the prefill uses.
//
//   y[M,N] = x[M,K] . w^T,  w[n][k] = e2m1(code[n][k]) * 2^(scale[n][k/32]-127)
//   x, y bf16. code: [N, K/2] bytes in the nn.Linear layout, element k in
//   byte k / 2, even k in the low nibble; a nibble is sign | e2m1 (0, 0.5, 1,
//   1.5, 2, 3, 4, 6). scale: [N, K/32] e8m0 bytes, each in [2, 254], so that
//   0.5 * 2^(byte-127) is a normal bf16 and every w is exactly a bf16 value.
//   Contract: 1 <= M <= 64, K % 128 == 0, N % 16 == 0.
//
//   linear_w4_kernel<MT>   grid (ceil(N/64), num_splits), 256 threads
//     The split of the work is linear_w8.hip's: MT = ceil(M/16) token tiles,
//     wave w of block (bx, z) owns channels n0 + 16w .. +15 (n0 = 64 bx) over
//     split z's run of the K/128 steps (q = steps / S, r = steps % S: split z
//     starts at z q + min(z, r) and has q + (z < r) steps; none: zero
//     partials, nothing read). A wave whose channels start at or past N
//     streams row N - 1 and stores nothing.
//
// Products, mfma_f32_16x16x32_bf16, four per 128-step; operand layouts as in
// linear_w8.hip (A: lane (i = lane & 15, g = lane >> 4) holds row i, k-slots
// 8g..8g+7; B: column i; C: column i, rows 4g..4g+3). W is A, x is B.
//   W stream: global -> VGPR, never through LDS. ONE 16-byte load per lane
//   and step = 32 codes = exactly one scale block: lane (i, g) takes bytes
//   16g .. 16g+15 of its row's 64-byte step, the four g-lanes of a row cover
//   the contiguous 64 bytes. Dword m of the load feeds MFMA m: k-slot e of
//   lane (i, g) in MFMA m is
//       k = 32 g + 8 m + e,
//   and the x fragments use the same map.
//   Widening: v_cvt_scalef32_pk_bf16_fp4, one per byte (op_sel picks the
//   byte; low nibble -> element 0), with the block scale as the scale
//   operand: 16 VALU instructions per 16-byte load, as many as w8 spends on
//   16 bytes, over twice the k. A power of two times an e2m1 value is a bf16
//   value: the MFMA operand is exactly w, nothing is rounded before the fp32
//   accumulator, and there is no scale multiply anywhere (none in the
//   epilogue either).
//   Scales: lane (i, g) needs byte g of its row's four scale bytes of the
//   step. Deviation from the issue's dword: a global_load_ubyte of exactly
//   that byte, issued with the W load it belongs to, four steps ahead; same
//   instruction count, no extract. scale = as_float(byte << 23), one shift,
//   valid because byte >= 2 (byte 0 would be a zero, 1 a denormal scale).
//
// Step width: 128 k was built, not 256. A 256-step wants steps in pairs and
// K % 128 == 0 allows an odd count, so every split would need a half step;
// the bytes in flight were raised by depth instead (below).
//
// Pipeline. Four W register sets, the loop unrolled by four so the sets have
// fixed names; W(t+4) and its scale byte are loaded into W(t)'s set right
// after W(t) was widened. The prologue issues W(0..3): 64 bytes per lane are
// in flight before the first is consumed, as in w8. x is staged two steps
// ahead into THREE LDS buffers (w8: one ahead, two buffers): vmcnt retires in
// order, so the wait for x(t) also completes every W load issued before it,
// and with x only one step ahead a deeper W queue would be drained at every
// step. Per step, in this order:
//     s_waitcnt vmcnt(MT + 4)   x(t) landed in this wave. Behind it in the
//                               queue and free to stay in flight: W, scale
//                               (t+2); the MT DMAs of x(t+1); W, scale (t+3)
//     barrier                   x(t) landed in every wave, and every wave is
//                               done reading buffer (t+2) % 3 (step t-1)
//     widen W(t)                its data arrived at the wait above
//     DMA x(t+2), load W(t+4)   in that order, pinned by sched_barrier
//     ds_read x(t), MFMAs
// One barrier per step. Inside the loop every step issues the same loads:
// past the split's end x is the last tile again and W, scale come from a
// padding line (the tensor's first 64 bytes; never consumed), so
// vmcnt(MT + 4) is exact. The up to three explicit tail steps after the loop
// load no W; the first still waits vmcnt(MT + 4), the second (MT + 2), the
// third (MT): two loads fewer behind x(t) each time.
// `code` and `scale` are not __restrict__ (deviation from the issue, the
// reason is w8's): the "memory" asm statements then fence the W loads and
// the counts above are the counts in the ISA.
//
// x staging and LDS image: linear_w8.hip's. [16 MT tokens][128 k] bf16 per
// step by 16-byte global -> LDS DMA (inline-asm form), wave w's instruction
// q writes rows 4(4q + w) .. +3, source row min(row, M - 1). A tile row is
// 256 bytes = sixteen 16-byte chunks = one bank row. The fragment read of
// MFMA m takes chunk c = 4g + m of row i (k = 32g + 8m .. +7): the 16 lanes
// served together are rows 0..15 of ONE chunk. Chunk c of row r is stored at
// slot c ^ (r & 15): for fixed c the slots of rows 0..15 are a bijection of
// 0..15, all 64 banks once: conflict-free, by w8's argument unchanged (it
// only needs "one chunk, sixteen rows"). The XOR is applied to the DMA's
// global source chunk and again to the read.
//
// Epilogue. num_splits == 1: round once to bf16, one 8-byte store of
// y[token][n .. n+3] per lane and tile. num_splits > 1: fp32 partials to
// ws[split][M][N] and w8's combine kernel (tok_split_combine) adds them in
// split order, 0 first, and rounds once. No atomics, every sum in a fixed
// order, the grid depends on shapes alone, and a token's row does not depend
// on its batch slot.
// fp32 budget (tests/test_linear_w4_gpu.py counts k from this): one MFMA
// chain over the split's products, at most 128 * ceil(steps / S) terms, one
// rounding per term; S - 1 adds in the combine. No scale unit.
//
//   w4_dequant_kernel   grid-stride, 256 threads
//     out[N,K] bf16 = w, exact: one 16-byte load (a scale block), its scale
//     byte, 16 converts, four 16-byte stores per thread. Serves M > 64 (the
//     prefill): dequantize, then the library GEMM of the bf16 path.
//
// Resources (hipcc -O3 --offload-arch=gfx950,
// -Rpass-analysis=kernel-resource-usage; scratch is 0 B everywhere):
//   kernel                     VGPR  AGPR  SGPR  LDS B  waves/SIMD
//   linear_w4_kernel<1>          60     4    39  12288  8
//   linear_w4_kernel<2>          62    12    39  24576  6
//   linear_w4_kernel<3>          66    16    39  36864  4
//   linear_w4_kernel<4>          72    24    39  49152  3
//   w4_dequant_kernel            23     0    22      0  8
// (the combine kernel is linear_w8.hip's.)
// ISA read (--save-temps): each loop step has the written vmcnt(MT + 4)
// before the barrier and, after it, the compiler's own vmcnt(6) for W(t): it
// counts the six W and scale loads behind W(t) and not the DMAs. For MT <= 2
// that is no wait at all; for MT = 3 / 4 it is stronger than the written one
// by one / two entries, so W, scale (t+2) are complete one step early there
// (M > 32 only). The tail steps have (MT + 4), (MT + 2), (MT); the only
// vmcnt(0) is the one after the last step, and no wait sits next to a
// global_load. The W sets are kept live to the end of the loop region, else
// a tail step reuses the register of a padding load in flight and the
// compiler waits vmcnt(0) for it.
#include "common.h"

#include <type_traits>

extern "C" hipError_t tok_split_combine(const float* ws, void* y, long nvec,
                                        int num_splits, hipStream_t stream);

namespace {

#if defined(__HIP_DEVICE_COMPILE__)
#define W4_KERNEL __global__ __attribute__((target("no-packed-fp32-ops")))
#else
#define W4_KERNEL __global__
#endif

using bf16x8v = __attribute__((ext_vector_type(8))) __bf16;
using bf16x2v = __attribute__((ext_vector_type(2))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;

constexpr int W4_NTH = 256;
constexpr int W4_BN = 64;          // output channels per block
constexpr int W4_KS = 128;         // k per step
constexpr int W4_WS = W4_KS / 2;   // code bytes of one row per step
constexpr int W4_ROW = W4_KS * 2;  // bytes of one x tile row
constexpr int W4_NBUF = 3;         // x buffers
constexpr int W4_SETS = 4;         // W register sets = steps W runs ahead

// 16 bytes per lane, global -> LDS: lane i's bytes land at lds_dst + 16 i.
DEVINL void w4_glds16(uint32_t voff, const void* sbase, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_dst)
      : "memory");
}

DEVINL void w4_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

DEVINL uint32_t w4_pack(float lo, float hi) {
  const f32x2 f = {lo, hi};
  union { bf16x2v b; uint32_t u; } c;
  c.b = __builtin_convertvector(f, bf16x2v);
  return c.u;
}

// e8m0 byte (>= 2) -> the power of two it stands for
DEVINL float w4_scale(uint32_t byte) {
  union { uint32_t u; float f; } c;
  c.u = byte << 23;
  return c.f;
}

// 8 e2m1 codes (one dword) * scale -> 8 bf16, nibble j = element j; exact
DEVINL bf16x8v w4_widen(uint32_t d, float scale) {
  union { bf16x2v p[4]; bf16x8v f; } r;
  r.p[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 0);
  r.p[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 1);
  r.p[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 2);
  r.p[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 3);
  return r.f;
}

template <int MT>
W4_KERNEL __launch_bounds__(W4_NTH) void linear_w4_kernel(
    const bf16_t* __restrict__ x, const uint8_t* code, const uint8_t* scale,
    bf16_t* __restrict__ y, float* __restrict__ ws, int M, int N, int K) {
  constexpr int TILE = MT * 16 * W4_ROW;  // one x buffer
  __shared__ __attribute__((aligned(1024))) char smem[W4_NBUF * TILE];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int z = blockIdx.y, S = gridDim.y;
  const int nw = blockIdx.x * W4_BN + wid * 16;  // the wave's first channel
  const bool live = nw < N;                      // wave-uniform

  const int steps = K / W4_KS;
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
    const char* xs = reinterpret_cast<const char*>(x) + (long)s0 * W4_ROW;

    // ---- fragment read offsets within a tile row block ----
    uint32_t b_off[4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
      b_off[m] = li * W4_ROW + 16 * ((4 * lg + m) ^ li);

    // ---- the lane's W row (a wave with no channels streams row N - 1) ----
    const long row = min(nw + li, N - 1);
    const uint8_t* wrow = code + row * (K / 2) + (long)s0 * W4_WS + 16 * lg;
    const uint8_t* srow = scale + row * (K / 32) + (long)s0 * 4 + lg;
    // a step past the split's end loads the padding line instead
    const uint8_t* wpad = code + 16 * lg;
    const uint8_t* spad = scale + lg;

    uint4 wr[W4_SETS];
    uint32_t sb[W4_SETS];
    auto load_w = [&](int u, int t) __attribute__((always_inline)) {
      const bool in = t < ns;
      wr[u] = *reinterpret_cast<const uint4*>(in ? wrow + (long)t * W4_WS
                                                 : wpad);
      sb[u] = *(in ? srow + (long)t * 4 : spad);
      asm volatile("" ::: "memory");
    };
    auto dma_x = [&](int t, int buf) __attribute__((always_inline)) {
      // the tile after the last is the last again; nobody reads it
      const char* src = xs + (long)min(t, ns - 1) * W4_ROW;
      const uint32_t dst = lds0 + buf * TILE;
#pragma unroll
      for (int q = 0; q < MT; ++q) w4_glds16(d_off[q], src, dst + q * 4096);
    };

    // prologue, ending in the loop's order: x(0), W(2), x(1), W(3)
    load_w(0, 0);
    load_w(1, 1);
    __builtin_amdgcn_sched_barrier(0);
    dma_x(0, 0);
    __builtin_amdgcn_sched_barrier(0);
    load_w(2, 2);
    __builtin_amdgcn_sched_barrier(0);
    dma_x(1, 1);
    __builtin_amdgcn_sched_barrier(0);
    load_w(3, 3);
    __builtin_amdgcn_sched_barrier(0);

    int cur = 0;  // t % 3, the buffer of x(t)
    // One step, a single basic block: u names the register set of W(t).
    // tail 0 is a step of the loop; tail j > 0 is the j-th step after it.
    // The tail steps load no W (nothing would consume it), so each finds
    // two loads fewer behind x(t) than the one before.
    auto step = [&](auto uc, auto tc, int t) __attribute__((always_inline)) {
      constexpr int u = decltype(uc)::value;
      constexpr int tail = decltype(tc)::value;
      // x(t) landed in this wave; (t+2)'s W, x(t+1), (t+3)'s W may fly on
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(
                       MT + 4 - 2 * (tail > 1 ? tail - 1 : 0))
                   : "memory");
      w4_barrier();

      const float sc = w4_scale(sb[u]);
      bf16x8v a[4];
      a[0] = w4_widen(wr[u].x, sc);
      a[1] = w4_widen(wr[u].y, sc);
      a[2] = w4_widen(wr[u].z, sc);
      a[3] = w4_widen(wr[u].w, sc);
      // volatile asm keeps its order: the widening stays above the DMA and
      // above the load that overwrites its register set
      asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]));
      __builtin_amdgcn_sched_barrier(0);
      dma_x(t + 2, cur == 0 ? 2 : cur - 1);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (tail == 0) load_w(u, t + 4);
      __builtin_amdgcn_sched_barrier(0);
      const char* xt = smem + cur * TILE;
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          union { uint4 u; bf16x8v f; } b;
          b.u = *reinterpret_cast<const uint4*>(xt + mt * 16 * W4_ROW +
                                                b_off[m]);
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m], b.f, acc[mt],
                                                            0, 0, 0);
        }
      cur = cur == 2 ? 0 : cur + 1;
      __builtin_amdgcn_sched_barrier(0);
    };
    using C0 = std::integral_constant<int, 0>;
    using C1 = std::integral_constant<int, 1>;
    using C2 = std::integral_constant<int, 2>;
    using C3 = std::integral_constant<int, 3>;

    int t = 0;
    for (; t + 4 <= ns; t += 4) {
      step(C0{}, C0{}, t);
      step(C1{}, C0{}, t + 1);
      step(C2{}, C0{}, t + 2);
      step(C3{}, C0{}, t + 3);
    }
    if (t < ns) step(C0{}, C1{}, t);
    if (t + 1 < ns) step(C1{}, C2{}, t + 1);
    if (t + 2 < ns) step(C2{}, C3{}, t + 2);
    // the last steps' DMAs must not land in an LDS that is no longer ours
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // the sets stay live to here: a tail step must not reuse the register of
    // a padding load that is still in flight (the compiler would wait for it)
#pragma unroll
    for (int u = 0; u < W4_SETS; ++u)
      asm volatile("" ::"v"(wr[u].x), "v"(wr[u].y), "v"(wr[u].z),
                   "v"(wr[u].w), "v"(sb[u]));
  }

  if (!live) return;
  const int n = nw + 4 * lg;  // this lane's four channels
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int tok = 16 * mt + li;
    if (tok >= M) continue;
    const f32x4 v = acc[mt];
    if (S == 1) {
      *reinterpret_cast<uint2*>(y + (long)tok * N + n) =
          make_uint2(w4_pack(v[0], v[1]), w4_pack(v[2], v[3]));
    } else {
      *reinterpret_cast<f32x4v*>(ws + ((long)z * M + tok) * N + n) =
          f32x4v{{v[0], v[1], v[2], v[3]}};
    }
  }
}

// one scale block (16 code bytes) per thread; block i has scale byte i
W4_KERNEL void w4_dequant_kernel(const uint4* __restrict__ code,
                                 const uint8_t* __restrict__ scale,
                                 uint4* __restrict__ out, long nblk) {
  for (long i = (long)blockIdx.x * W4_NTH + threadIdx.x; i < nblk;
       i += (long)gridDim.x * W4_NTH) {
    const float s = w4_scale(scale[i]);
    const uint4 c = code[i];
    const uint32_t d[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      union { bf16x8v f; uint4 u; } o;
      o.f = w4_widen(d[j], s);
      out[4 * i + j] = o.u;
    }
  }
}

template <int MT>
void launch_w4(const void* x, const void* code, const void* scale, void* y,
               float* ws, int M, int N, int K, int num_splits,
               hipStream_t stream) {
  dim3 grid((N + W4_BN - 1) / W4_BN, num_splits);
  linear_w4_kernel<MT><<<grid, W4_NTH, 0, stream>>>(
      (const bf16_t*)x, (const uint8_t*)code, (const uint8_t*)scale,
      (bf16_t*)y, ws, M, N, K);
}

}  // namespace

extern "C" {

// code: [N, K/2] bytes; scale: [N, K/32] bytes; ws: fp32, num_splits*M*N
// elements, unused when num_splits == 1.
hipError_t tok_linear_w4(const void* x, const void* code, const void* scale,
                         void* y, float* ws, int M, int N, int K,
                         int num_splits, hipStream_t stream) {
  if (M < 1 || M > 64 || K < W4_KS || K % W4_KS != 0 || N < 16 ||
      N % 16 != 0 || num_splits < 1 || num_splits > 65535 ||
      (num_splits > 1 && ws == nullptr))
    return hipErrorInvalidValue;
  switch ((M + 15) / 16) {
    case 1: launch_w4<1>(x, code, scale, y, ws, M, N, K, num_splits, stream); break;
    case 2: launch_w4<2>(x, code, scale, y, ws, M, N, K, num_splits, stream); break;
    case 3: launch_w4<3>(x, code, scale, y, ws, M, N, K, num_splits, stream); break;
    default: launch_w4<4>(x, code, scale, y, ws, M, N, K, num_splits, stream); break;
  }
  HIP_CHECK(hipGetLastError());
  if (num_splits > 1)
    HIP_CHECK(tok_split_combine(ws, y, (long)M * N / 4, num_splits, stream));
  return hipSuccess;
}

hipError_t tok_w4_dequant(const void* code, const void* scale, void* out,
                          long N, int K, hipStream_t stream) {
  if (N < 1 || K < 32 || K % 32 != 0) return hipErrorInvalidValue;
  const long nblk = N * (K / 32);
  long grid = (nblk + W4_NTH - 1) / W4_NTH;
  if (grid > 8192) grid = 8192;
  w4_dequant_kernel<<<(int)grid, W4_NTH, 0, stream>>>(
      (const uint4*)code, (const uint8_t*)scale, (uint4*)out, nblk);
  return hipGetLastError();
}
}
