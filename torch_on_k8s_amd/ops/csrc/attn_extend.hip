// Chunked ragged prefill for MI355X (gfx950): Tq new tokens per sequence,
// causal among themselves, against a ragged KV-cache prefix; and the
// multi-token append that goes with it.
//
//   attn_extend_kernel<D, R>   grid (Hkv * ceil(Tq*R/64), B, num_splits), 256 thr
//     q [B,Tq,Hq,D], kcache/vcache [B,Tmax,Hkv,D] (the new tokens' K/V already
//     appended), lens/qlens [B] int32 on the device.
//     n = clamp(lens[b], 0, Tmax), m = clamp(qlens[b], 0, min(Tq, n)); query
//     i < m sits at p_i = n - m + i and attends to cache rows [0, p_i]; rows
//     i >= m are exactly zero and read nothing.
//
// Work split. The M dimension packs (token, head of the group) as
// row = i*R + r: a 64-row tile is 64/R consecutive tokens of ONE kv head, so
// all R query heads share one read of K and V. Four waves of 16 rows each.
// Split z owns keys [z*chunk, (z+1)*chunk) clipped to p_last + 1, the limit of
// the block's last live row. A block whose first token is >= m, or whose
// chunk starts past p_last, is block-uniformly dead: it writes zeros (or
// m = -inf, l = 0 partials) and returns, as the decode kernel's empty chunk.
//
// Key loop. 64-key tiles. K and V tiles go global -> LDS by 16-byte DMA
// (global_load_lds_dwordx4, the inline-asm form of wgrad_gemm.hip: the builtin
// forces vmcnt(0)), two buffers: tile t+1 is issued, then vmcnt(NDMA) says
// tile t has landed in this wave and a barrier says so of every wave; a
// second barrier after the MFMAs frees the buffer for tile t+2. A tile past
// the chunk's end is the last tile again (nobody reads it; the count stays
// uniform). The DMA source row is min(key, kend - 1): a row past n never
// enters LDS (0 * NaN inside an MFMA is NaN).
//
// Products, mfma_f32_16x16x32_bf16. A operand: lane (i = lane & 15,
// g = lane >> 4) holds row i, k-slots 8g..8g+7; B operand: column i, the same
// k-slots; C: column i, rows 4g..4g+3.
//   S^T = K Q^T   A = K rows (key 16kt + i, d = 32ks + 8g ..): one 16-byte LDS
//                 read; B = Q (q row i), resident in registers for the whole
//                 loop. C: lane holds q row i, keys 16kt + 4g + j.
//   O = P V       A = P: k-slot e of lane (i, g) of the 32-key step kk IS the
//                 accumulator st[2kk + (e >> 2)][e & 3] of that lane, i.e.
//                 key 32kk + 16(e >> 2) + 4g + (e & 3): the score layout is
//                 the operand layout and P never moves. B = V[key][d] with
//                 the same slot -> key map: V stays row-major [key][d] in LDS
//                 and ds_read_b64_tr_b16 hands lane i column d = 16dt + i of
//                 the four keys 32kk + 16u + 4g + 0..3 (u = e >> 2).
//                 C: lane holds d = 16dt + i, q rows 4g + j.
// So a lane owns ONE q row's scores (row statistics: an in-lane chain and
// two shuffles over g) and four q rows' outputs; alpha and 1/l cross by one
// shuffle per j per tile.
//
// LDS image of a tile: row r (D*2 bytes), 16-byte chunk ch at slot
// ch ^ f(r & 15). The DMA writes LDS linearly (wave base + 16 lane), so the
// XOR is applied to the global SOURCE chunk and again to the read address.
// Bank rule: bank = (addr / 4) % 64, i.e. a 256-byte bank row of sixteen
// 16-byte slots; a b128 read is served 16 lanes at a time, a transposed b64
// read conflicts within a 32-lane half.
//   D = 128 (256-byte rows, 16 chunks): f(r) = (r&3)<<2 | ((r>>2)&1)<<1 | r>>3.
//     K read: 16 lanes = rows 16kt + 0..15 of one chunk c: slots c ^ f(r), f a
//       bit permutation of 0..15: 16 distinct slots.
//     V read: a half is groups g0, g0+1: rows r = 4g + q, chunks 2dt + b
//       (b = p >> 1): slot = (2dt + b) ^ f(r): bit 0 from b (f's bit 0 is r>>3,
//       constant in a half), bit 1 from g & 1, bits 2-3 from q: 16 distinct.
//   D = 64 (128-byte rows, 8 chunks; a bank row is rows 2a, 2a+1):
//     f(r) = ((r>>1)&1)<<2 | ((r>>2)&1)<<1 | r>>3; bank slot = 8(r&1) + (ch^f).
//     K read: bit 3 from r&1, bits 0-2 from f, a bijection of r>>1: distinct.
//     V read: bit 3 from q&1, bit 2 from q>>1, bit 1 from g&1, bit 0 from b.
//
// Softmax: online, log2 domain, p = exp2(fma(s, scale*log2e, -m*scale*log2e)).
// A wave compares against the row limits only on tiles that reach past its
// first row's limit; there a masked score becomes -inf and its p 0 by select.
// Dead rows of a live block run with q = 0 (finite scores) and are zeroed by
// select at the end. l sums the unrounded p per lane; the four lanes of a row
// are added in g order at the end. P is rounded to bf16 once, for P.V.
//
// Epilogue: num_splits == 1 normalises and writes bf16 rows as 16-byte
// stores through LDS; otherwise fp32 (m, l, o[D]) partials in the workspace
// layout of attn_decode_ragged_combine with rows = B*Tq*Hq, which folds them
// in split order. No atomics, every sum in a fixed order; the grid depends
// on shapes alone: capturable, bitwise repeatable, slot-independent.
//
//   qkv_rope_append_chunk_kernel   grid-stride, 256 threads
//     qkv [B,Tq,(Hq+2Hkv)*D]: token i of sequence b is rotated at pos[b] + i
//     and its k, v written to cache[b, pos[b] + i]; live iff i < qlens[b] and
//     0 <= pos[b] + i < Tmax; a dead token gets a zero q row and writes
//     nothing. Per element as qkv_rope_append_kernel: fp32, two products and
//     an add.
//
// Resources (hipcc -O3 --offload-arch=gfx950,
// -Rpass-analysis=kernel-resource-usage; scratch is 0 B everywhere):
//   kernel                         VGPR  SGPR  LDS B  waves/SIMD
//   attn_extend_kernel<128,1>       132    52  65536  2
//   attn_extend_kernel<128,2|4|8>   132    54  65536  2
//   attn_extend_kernel<64,1>         92    52  32768  5
//   attn_extend_kernel<64,2|4|8>     92    54  32768  5
//   qkv_rope_append_chunk_kernel     51    70      0  8
// (waves/SIMD is the register figure; LDS allows two blocks = 2 waves/SIMD at
// D = 128 and five blocks at D = 64.)
#include "common.h"

extern "C" hipError_t tok_attn_ragged_combine(const float* ws, void* out,
                                              int rows, int Hq, int D,
                                              int num_splits,
                                              hipStream_t stream);

namespace {

#if defined(__HIP_DEVICE_COMPILE__)
#define EXT_KERNEL __global__ __attribute__((target("no-packed-fp32-ops")))
#else
#define EXT_KERNEL __global__
#endif

using bf16x8v = __attribute__((ext_vector_type(8))) __bf16;
using bf16x2v = __attribute__((ext_vector_type(2))) __bf16;
using i16x4v = __attribute__((ext_vector_type(4))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;

constexpr int EX_NTH = 256;
constexpr int EX_BM = 64;   // packed q rows per block
constexpr int EX_BN = 64;   // keys per tile
constexpr float EX_LOG2E = 1.4426950408889634f;

typedef __attribute__((address_space(3))) i16x4v* ex_tr_ptr;

DEVINL i16x4v ex_tr_read(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((ex_tr_ptr)p);
}

// 16 bytes per lane, global -> LDS: lane i's bytes land at lds_dst + 16 i.
DEVINL void ex_glds16(uint32_t voff, const void* sbase, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_dst)
      : "memory");
}

DEVINL void ex_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

template <int D>
DEVINL int ex_swz(int r) {
  if (D == 128)
    return ((r & 3) << 2) | (((r >> 2) & 1) << 1) | ((r >> 3) & 1);
  return (((r >> 1) & 1) << 2) | (((r >> 2) & 1) << 1) | ((r >> 3) & 1);
}

DEVINL uint32_t ex_pack(float lo, float hi) {
  const f32x2 f = {lo, hi};
  union { bf16x2v b; uint32_t u; } c;
  c.b = __builtin_convertvector(f, bf16x2v);
  return c.u;
}

// packed row (token i, head r of the group) = i*R + r -> index in [B*Tq*Hq]
template <int R>
struct ExRows {
  long tok0;   // b * Tq
  int Hq, h0;  // h0 = hkv * R
  DEVINL long global(int row) const {
    return (tok0 + row / R) * Hq + h0 + row % R;
  }
};

// One K and one V tile, keys k0 .. k0 + 63 clamped to klast, into the pair of
// tiles at LDS address dst (wave part included).
template <int D>
DEVINL void ex_stage(const char* kbase, const char* vbase, uint32_t dst,
                     int k0, int klast, int d_row, int d_ch,
                     uint32_t row_bytes) {
  constexpr int TILE = EX_BN * D * 2, NJ = TILE / 4096, RPS = 4096 / (D * 2);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int key = min(k0 + j * RPS + d_row, klast);
    const uint32_t voff = (uint32_t)key * row_bytes + d_ch * 16;
    ex_glds16(voff, kbase, dst + j * 4096);
    ex_glds16(voff, vbase, dst + TILE + j * 4096);
  }
}

template <int D, int R>
EXT_KERNEL __launch_bounds__(EX_NTH, 2) void attn_extend_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ kc,
    const bf16_t* __restrict__ vc, const int* __restrict__ lens,
    const int* __restrict__ qlens, bf16_t* __restrict__ out,
    float* __restrict__ ws, int Tq, int Tmax, int Hkv, int MT, int chunk,
    float scale) {
  constexpr int RB = D * 2;                    // bytes per tile row
  constexpr int TILE = EX_BN * RB;             // one K or V tile
  constexpr int NJ = TILE / 4096;              // DMA instructions per tile
  constexpr int CPR = D / 8;                   // 16-byte chunks per row
  constexpr int KS = D / 32;                   // k steps of S^T
  constexpr int DT = D / 16;                   // d tiles of O
  constexpr int OLD = D + 8;                   // epilogue row, bf16 elements
  __shared__ __attribute__((aligned(1024))) char smem[4 * TILE];
  static_assert(4 * 16 * OLD * 2 <= 4 * TILE, "epilogue image fits");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int hkv = blockIdx.x / MT, mt = blockIdx.x - hkv * MT;
  const int b = blockIdx.y, sp = blockIdx.z;
  const int S = gridDim.z;
  const int Hq = Hkv * R;
  const int NR = Tq * R;                       // packed rows of this kv head

  const int n = min(max(lens[b], 0), Tmax);
  const int m = min(max(qlens[b], 0), min(Tq, n));
  const int base_pos = n - m;                  // position of query 0

  const int row_blk = mt * EX_BM;
  const int i_first = row_blk / R;
  const int i_last = min(m - 1, (row_blk + EX_BM - 1) / R);
  const int p_last = base_pos + i_last;
  const int kbeg = sp * chunk;
  const int kend = min(kbeg + chunk, p_last + 1);

  const ExRows<R> rows{(long)b * Tq, Hq, hkv * R};
  const long ws_ml0 = (long)gridDim.y * Tq * Hq * S * D;

  if (i_first >= m || kbeg >= kend) {  // block-uniform: nothing to attend to
    for (int idx = tid; idx < EX_BM * CPR; idx += EX_NTH) {
      const int row = row_blk + idx / CPR, ch = idx % CPR;
      if (row >= NR) continue;
      const long gr = rows.global(row);
      if (S == 1) {
        bf16x8 z;
#pragma unroll
        for (int j = 0; j < 8; ++j) z.h[j] = 0;
        *reinterpret_cast<bf16x8*>(out + gr * D + ch * 8) = z;
      } else {
        const f32x4v z = {{0.f, 0.f, 0.f, 0.f}};
        float* po = ws + (gr * S + sp) * D + ch * 8;
        reinterpret_cast<f32x4v*>(po)[0] = z;
        reinterpret_cast<f32x4v*>(po)[1] = z;
        if (ch == 0) {
          ws[ws_ml0 + (gr * S + sp) * 2] = -INFINITY;
          ws[ws_ml0 + (gr * S + sp) * 2 + 1] = 0.f;
        }
      }
    }
    return;
  }

  // ---- this wave's rows ----
  const int row_w = row_blk + wid * 16;               // wave's first row
  const bool wave_live = row_w < NR && row_w / R < m;  // wave-uniform
  const int lim_first = base_pos + row_w / R;
  const int lim_last = base_pos + min(m - 1, (row_w + 15) / R);
  const int row_s = row_w + li;                        // the lane's score row
  const bool live_s = row_s < NR && row_s / R < m;
  const int lim_s = live_s ? base_pos + row_s / R : -1;

  // Q as the B operand of S^T, resident. A dead row loads nothing: zeros.
  bf16x8v qf[KS];
  {
    const bf16_t* qrow = q + rows.global(live_s ? row_s : row_blk) * D + lg * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      uint4 raw = {0, 0, 0, 0};
      if (live_s) raw = *reinterpret_cast<const uint4*>(qrow + ks * 32);
      union { uint4 u; bf16x8v f; } c;
      c.u = raw;
      qf[ks] = c.f;
    }
  }

  // ---- DMA geometry ----
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane(
      (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem +
      wid * 1024);
  const int d_row = tid / CPR;                         // row within a slab
  const int d_ch = (tid % CPR) ^ ex_swz<D>(d_row & 15);
  const uint32_t row_bytes = (uint32_t)Hkv * D * 2;    // between cache rows
  const long head_off = ((long)b * Tmax * Hkv + hkv) * D;
  const char* kbase = reinterpret_cast<const char*>(kc + head_off);
  const char* vbase = reinterpret_cast<const char*>(vc + head_off);
  const int ntiles = (kend - kbeg + EX_BN - 1) / EX_BN;


  // ---- fragment read offsets (bytes within a tile) ----
  uint32_t k_off[KS];   // + kt * 16 * RB
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
    k_off[ks] = li * RB + 16 * ((4 * ks + lg) ^ ex_swz<D>(li));
  // transposed read: lane 4q+p of group g supplies row 16u + 4g + q (+ 32kk),
  // columns 16dt + 4p .. + 3: chunk 2dt + (p >> 1), half p & 1
  uint32_t v_base[2], v_x[2];
  {
    const int tq = (lane >> 2) & 3, tp = lane & 3;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = 16 * u + 4 * lg + tq;
      v_base[u] = r * RB + 8 * (tp & 1);
      v_x[u] = (tp >> 1) ^ ex_swz<D>(r & 15);
    }
  }

  const float c2 = scale * EX_LOG2E;
  float m_run = -INFINITY, l_run = 0.f;
  f32x4 o_acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o_acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  ex_stage<D>(kbase, vbase, lds0, kbeg, kend - 1, d_row, d_ch, row_bytes);
  for (int t = 0; t < ntiles; ++t) {
    const int buf = t & 1;
    ex_stage<D>(kbase, vbase, lds0 + (buf ^ 1) * 2 * TILE,
                kbeg + min(t + 1, ntiles - 1) * EX_BN, kend - 1, d_row, d_ch,
                row_bytes);
    if (NJ == 4)
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    ex_barrier();

    const int k0 = kbeg + t * EX_BN;
    if (wave_live && k0 <= lim_last) {
      const char* kt_lds = smem + buf * 2 * TILE;
      const char* vt_lds = kt_lds + TILE;

      // S^T = K Q^T: st[kt][j] = score of (key k0 + 16kt + 4g + j, row li)
      f32x4 st[4];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        st[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          union { uint4 u; bf16x8v f; } a;
          a.u = *reinterpret_cast<const uint4*>(kt_lds + kt * 16 * RB +
                                                k_off[ks]);
          st[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.f, qf[ks],
                                                           st[kt], 0, 0, 0);
        }
      }

      const bool needs_mask = k0 + EX_BN - 1 > lim_first;  // wave-uniform
      if (needs_mask) {
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            st[kt][j] = (k0 + 16 * kt + 4 * lg + j <= lim_s) ? st[kt][j]
                                                             : -INFINITY;
      }

      float tmax = st[0][0];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) tmax = fmaxf(tmax, st[kt][j]);
      tmax = fmaxf(tmax, __shfl_xor(tmax, 16, WAVE));
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, WAVE));
      const float m_new = fmaxf(m_run, tmax);
      // a row with no key yet keeps m = -inf; its exponent offset is 0, so
      // that exp2(-inf + 0) is 0 and never exp2(-inf + inf)
      const float neg_mc = (m_new == -INFINITY) ? 0.f : -m_new * c2;
      const float alpha =
          __builtin_amdgcn_exp2f(__builtin_fmaf(m_run, c2, neg_mc));
      m_run = m_new;

      float psum = 0.f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float p = __builtin_amdgcn_exp2f(
              __builtin_fmaf(st[kt][j], c2, neg_mc));
          if (needs_mask)
            p = (k0 + 16 * kt + 4 * lg + j <= lim_s) ? p : 0.f;
          st[kt][j] = p;
          psum += p;
        }
      l_run = __builtin_fmaf(l_run, alpha, psum);

      // P as the A operand: one rounding to bf16
      bf16x8v pa[2];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        union { uint32_t w[4]; bf16x8v f; } c;
        c.w[0] = ex_pack(st[2 * kk][0], st[2 * kk][1]);
        c.w[1] = ex_pack(st[2 * kk][2], st[2 * kk][3]);
        c.w[2] = ex_pack(st[2 * kk + 1][0], st[2 * kk + 1][1]);
        c.w[3] = ex_pack(st[2 * kk + 1][2], st[2 * kk + 1][3]);
        pa[kk] = c.f;
      }

      // alpha of output row 4g + j lives in lane 4g + j
      float al[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) al[j] = __shfl(alpha, 4 * lg + j, WAVE);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int j = 0; j < 4; ++j) o_acc[dt][j] *= al[j];

#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          union { i16x4v s[2]; bf16x8v f; } vb;
#pragma unroll
          for (int u = 0; u < 2; ++u)
            vb.s[u] = ex_tr_read(vt_lds + kk * 32 * RB + v_base[u] +
                                 16 * ((2 * dt) ^ v_x[u]));
          o_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              pa[kk], vb.f, o_acc[dt], 0, 0, 0);
        }
    }
    ex_barrier();
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  ex_barrier();

  // ---- row sums: the four lanes of a row, in g order ----
  float l_row = 0.f;
#pragma unroll
  for (int g = 0; g < 4; ++g) l_row += __shfl(l_run, li + 16 * g, WAVE);
  if (!live_s || !wave_live) {   // dead rows: no state, by select
    l_row = 0.f;
    m_run = -INFINITY;
  }

  if (S == 1) {
    const float inv = (l_row > 0.f) ? 1.f / l_row : 0.f;
    bf16_t* img = reinterpret_cast<bf16_t*>(smem) + wid * 16 * OLD;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float ij = __shfl(inv, 4 * lg + j, WAVE);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const float val = (ij > 0.f) ? o_acc[dt][j] * ij : 0.f;
        img[(4 * lg + j) * OLD + dt * 16 + li] = f2bf(val);
      }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 16 * CPR / WAVE; ++it) {
      const int idx = it * WAVE + lane;
      const int r = idx / CPR, ch = idx % CPR;
      const int row = row_w + r;
      if (row < NR)
        *reinterpret_cast<uint4*>(out + rows.global(row) * D + ch * 8) =
            *reinterpret_cast<const uint4*>(img + r * OLD + ch * 8);
    }
  } else {
    // partial (m in natural-log units, l, unnormalised o)
    const float m_nat = (m_run == -INFINITY) ? -INFINITY : m_run * scale;
    if (lg == 0 && row_s < NR) {
      const long gr = rows.global(row_s);
      ws[ws_ml0 + (gr * S + sp) * 2] = m_nat;
      ws[ws_ml0 + (gr * S + sp) * 2 + 1] = l_row;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float lj = __shfl(l_row, 4 * lg + j, WAVE);
      const int row = row_w + 4 * lg + j;
      if (row < NR) {
        float* po = ws + (rows.global(row) * S + sp) * D + li;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
          po[dt * 16] = (lj > 0.f) ? o_acc[dt][j] : 0.f;
      }
    }
  }
}

constexpr int BLOCK_APPC = 256;

// Work item = one 8-wide vec of the first half of one head row of one token
// and its partner in the second half, as qkv_rope_append_kernel.
EXT_KERNEL void qkv_rope_append_chunk_kernel(
    const bf16x8* __restrict__ qkv, bf16x8* __restrict__ q,
    bf16x8* __restrict__ kcache, bf16x8* __restrict__ vcache,
    const float* __restrict__ tab_cos, const float* __restrict__ tab_sin,
    const int* __restrict__ pos, const int* __restrict__ qlens, int B, int Tq,
    int Tmax, int Hq, int Hkv, int hv /* (D/2)/8 */) {
  const int heads_total = Hq + 2 * Hkv;
  const int dv8 = hv * 2;  // vecs per head (D/8)
  const long nwork = (long)B * Tq * heads_total * hv;
  for (long i = (long)blockIdx.x * BLOCK_APPC + threadIdx.x; i < nwork;
       i += (long)gridDim.x * BLOCK_APPC) {
    const long rowh = i / hv;                 // (b*Tq + t)*heads_total + h
    const int c = (int)(i - rowh * hv);
    const long tok = rowh / heads_total;      // b*Tq + t
    const int h = (int)(rowh - tok * heads_total);
    const int b = (int)(tok / Tq);
    const int t = (int)(tok - (long)b * Tq);
    const long p = (long)pos[b] + t;
    const bool live = t < qlens[b] && p >= 0 && p < Tmax;
    bf16x8* dst;
    bool rot;
    if (h < Hq) {
      dst = q + (tok * Hq + h) * dv8;
      rot = true;
      if (!live) {  // zero q row, caches untouched
        bf16x8 z;
#pragma unroll
        for (int j = 0; j < 8; ++j) z.h[j] = 0;
        dst[c] = z;
        dst[c + hv] = z;
        continue;
      }
    } else {
      if (!live) continue;
      const bool isk = h < Hq + Hkv;
      const int hh = isk ? h - Hq : h - Hq - Hkv;
      dst = (isk ? kcache : vcache) + (((long)b * Tmax + p) * Hkv + hh) * dv8;
      rot = isk;
    }
    const bf16x8* src = qkv + rowh * dv8;
    const bf16x8 x1 = src[c];
    const bf16x8 x2 = src[c + hv];
    if (rot) {
      const float* cosr = tab_cos + p * (hv * 8);
      const float* sinr = tab_sin + p * (hv * 8);
      bf16x8 o1, o2;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float cs = cosr[c * 8 + j];
        const float sn = sinr[c * 8 + j];
        const float a = bfbits2f(x1.h[j]);
        const float bb = bfbits2f(x2.h[j]);
        o1.h[j] = f2bfbits(a * cs - bb * sn);
        o2.h[j] = f2bfbits(bb * cs + a * sn);
      }
      dst[c] = o1;
      dst[c + hv] = o2;
    } else {
      dst[c] = x1;
      dst[c + hv] = x2;
    }
  }
}

template <int D, int R>
void launch_extend(const void* q, const void* k, const void* v,
                   const int* lens, const int* qlens, void* out, float* ws,
                   int B, int Tq, int Tmax, int Hkv, int num_splits, int chunk,
                   hipStream_t stream) {
  const int MT = (Tq * R + EX_BM - 1) / EX_BM;
  dim3 grid(Hkv * MT, B, num_splits);
  const float scale = 1.f / sqrtf((float)D);
  attn_extend_kernel<D, R><<<grid, EX_NTH, 0, stream>>>(
      (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, lens, qlens,
      (bf16_t*)out, ws, Tq, Tmax, Hkv, MT, chunk, scale);
}

template <int D>
bool launch_extend_r(int R, const void* q, const void* k, const void* v,
                     const int* lens, const int* qlens, void* out, float* ws,
                     int B, int Tq, int Tmax, int Hkv, int num_splits,
                     int chunk, hipStream_t stream) {
  switch (R) {
    case 1: launch_extend<D, 1>(q, k, v, lens, qlens, out, ws, B, Tq, Tmax,
                                Hkv, num_splits, chunk, stream); return true;
    case 2: launch_extend<D, 2>(q, k, v, lens, qlens, out, ws, B, Tq, Tmax,
                                Hkv, num_splits, chunk, stream); return true;
    case 4: launch_extend<D, 4>(q, k, v, lens, qlens, out, ws, B, Tq, Tmax,
                                Hkv, num_splits, chunk, stream); return true;
    case 8: launch_extend<D, 8>(q, k, v, lens, qlens, out, ws, B, Tq, Tmax,
                                Hkv, num_splits, chunk, stream); return true;
    default: return false;
  }
}

}  // namespace

extern "C" {

// ws: fp32, B*Tq*Hq*num_splits*(D+2) elements; unused when num_splits == 1.
hipError_t tok_attn_extend(const void* q, const void* k, const void* v,
                           const int* lens, const int* qlens, void* out,
                           float* ws, int B, int Tq, int Tmax, int Hq, int Hkv,
                           int D, int num_splits, int chunk,
                           hipStream_t stream) {
  if (Hkv < 1 || Hq % Hkv != 0 || Tq < 1 || num_splits < 1 ||
      chunk < EX_BN || chunk % EX_BN != 0 || (long)num_splits * chunk < Tmax ||
      (long)Tmax * Hkv * D * 2 >= (1L << 31))
    return hipErrorInvalidValue;
  const int R = Hq / Hkv;
  bool ok = false;
  if (D == 128)
    ok = launch_extend_r<128>(R, q, k, v, lens, qlens, out, ws, B, Tq, Tmax,
                              Hkv, num_splits, chunk, stream);
  else if (D == 64)
    ok = launch_extend_r<64>(R, q, k, v, lens, qlens, out, ws, B, Tq, Tmax,
                             Hkv, num_splits, chunk, stream);
  if (!ok) return hipErrorInvalidValue;
  HIP_CHECK(hipGetLastError());
  if (num_splits > 1)
    HIP_CHECK(tok_attn_ragged_combine(ws, out, B * Tq, Hq, D, num_splits,
                                      stream));
  return hipSuccess;
}

hipError_t tok_qkv_rope_append_chunk(const void* qkv, void* q, void* kcache,
                                     void* vcache, const float* cos_tab,
                                     const float* sin_tab, const int* pos,
                                     const int* qlens, int B, int Tq, int Tmax,
                                     int Hq, int Hkv, int D,
                                     hipStream_t stream) {
  const int hv = (D / 2) / 8;
  const long nwork = (long)B * Tq * (Hq + 2 * Hkv) * hv;
  long grid = (nwork + BLOCK_APPC - 1) / BLOCK_APPC;
  if (grid > 8192) grid = 8192;
  if (grid < 1) grid = 1;
  qkv_rope_append_chunk_kernel<<<(int)grid, BLOCK_APPC, 0, stream>>>(
      (const bf16x8*)qkv, (bf16x8*)q, (bf16x8*)kcache, (bf16x8*)vcache,
      cos_tab, sin_tab, pos, qlens, B, Tq, Tmax, Hq, Hkv, hv);
  return hipGetLastError();
}
}
