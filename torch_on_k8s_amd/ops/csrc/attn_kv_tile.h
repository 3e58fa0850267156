// The tile core of the KV-cache attention kernels for MI355X (gfx950), and the
// destinations of the appends that fill those caches: what attn_extend.hip
// (contiguous bf16 cache), attn_paged.hip (bf16 pages) and attn_paged_fp8.hip
// (e4m3 pages) share. attn_extend_kernel is kt_attn over a contiguous Src;
// attn_paged_fp8_kernel is composed of the segments below; attn_paged_kernel
// follows this design and uses the primitives, but still carries its own
// copy of the body (its header says why). PagedSrc-shaped sources fit
// kt_attn as it stands: the prefetch hook is for them.
//
// Contract of all three. q [B,Tq,Hq,D] bf16, lens/qlens [B] int32 on the
// device, grid (Hkv * row_tiles, B, num_splits), 256 threads.
// n = clamp(lens[b], 0, Tmax), m = clamp(qlens[b], 0, min(Tq, n)); query
// i < m sits at p_i = n - m + i and attends to cache rows [0, p_i]; rows
// i >= m are exactly zero and read nothing.
//
// Work split. The M dimension packs (token, head of the group) as
// row = i*R + r: a tile of packed rows is consecutive tokens of ONE kv head, so
// all R query heads share one read of K and V. Split z owns keys
// [z*chunk, (z+1)*chunk) clipped to p_last + 1, the limit of the block's last
// live row. A block whose first token is >= m, or whose chunk starts past
// p_last, is block-uniformly dead: it writes zeros (or m = -inf, l = 0
// partials) and returns.
//   Row layout (KEYSPLIT = false): 64 packed rows per block, four waves of 16
//     rows each; every wave runs all 64 keys of a tile (NKT = 4 groups of 16).
//   Key-split layout (KEYSPLIT = true, Tq * R <= 16; decode is Tq = 1): one
//     16-row tile for the block; wave w owns keys 16w .. 16w + 15 of every
//     tile (NKT = 1). Each wave keeps its own (m, l, o[D]) for the 16 rows
//     over all tiles of the split; at the end the four states go to LDS as
//     fp32 and 16 * D/8 threads fold them in wave order: M = max m_w,
//     e_w = exp2 of (m_w - M) in log2 units, L = fma(l_w, e_w, L),
//     o = fma(o_w, e_w, o). A wave's mask test uses its own 16 keys against
//     the row limits; a wave whose keys all lie past the last row's limit
//     skips the tile's arithmetic.
//
// Key loop. 64-key tiles. K and V tiles go global -> LDS by 16-byte DMA
// (global_load_lds_dwordx4, the inline-asm form of wgrad_gemm.hip: the builtin
// forces vmcnt(0)), two buffers: tile t+1 is issued, then one counted
// vmcnt(DMAs per tile) says tile t has landed in this wave and a barrier says
// so of every wave; a last barrier after the MFMAs frees the buffer for tile
// t+2. A tile past the chunk's end is the last tile again (nobody reads it;
// the count stays uniform). The DMA source row is min(key, kend - 1): a row
// past n never enters LDS (0 * NaN inside an MFMA is NaN). The compiler's own
// wait for the q loads would be a vmcnt(0) inside the loop (it does not count
// the inline-asm DMAs), so q is "used" by an empty asm before the loop.
//
// Products, mfma_f32_16x16x32_bf16. A operand: lane (i = lane & 15,
// g = lane >> 4) holds row i, k-slots 8g..8g+7; B operand: column i, the same
// k-slots; C: column i, rows 4g..4g+3.
//   S^T = K Q^T   A = K rows (key 16kt + i, d = 32ks + 8g ..): one 16-byte LDS
//                 read; B = Q (q row i), resident in registers for the whole
//                 loop. C: lane holds q row i, keys 16kt + 4g + j.
//   O = P V       A = P: k-slot e of lane (i, g) of the 32-key step kk IS the
//   (NKT = 4)     accumulator st[2kk + (e >> 2)][e & 3] of that lane, i.e.
//                 key 32kk + 16(e >> 2) + 4g + (e & 3): the score layout is
//                 the operand layout and P never moves. B = V[key][d] with
//                 the same slot -> key map: V stays row-major [key][d] in LDS
//                 and ds_read_b64_tr_b16 hands lane i column d = 16dt + i of
//                 the four keys 32kk + 16u + 4g + 0..3 (u = e >> 2).
//                 C: lane holds d = 16dt + i, q rows 4g + j.
//   O = P V       mfma_f32_16x16x16_bf16 on the wave's 16 keys: lane (i, g) of
//   (NKT = 1)     the S^T accumulator holds q row i, keys 4g .. 4g + 3, which
//                 is that instruction's A operand (row i, k-slots 4g .. + 3);
//                 one transposed b64 read hands lane (i, g) column 16dt + i of
//                 V rows 16w + 4g .. + 3, its B operand.
// So a lane owns ONE q row's scores (row statistics: an in-lane chain and
// two shuffles over g) and four q rows' outputs; alpha and 1/l cross by one
// shuffle per j per tile.
//
// LDS image of a bf16 tile: row r (D*2 bytes), 16-byte chunk ch at slot
// ch ^ f(r & 15), f = kt_swz. The DMA writes LDS linearly (wave base +
// 16 lane), so the XOR is applied to the global SOURCE chunk and again to the
// read address. Bank rule: bank = (addr / 4) % 64, i.e. a 256-byte bank row of
// sixteen 16-byte slots; a b128 read is served 16 lanes at a time, a
// transposed b64 read conflicts within a 32-lane half.
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
//   The key-split reads take K rows 16w + 0..15 (one chunk) and V rows
//   16w + 4g + q instead of 16kt + .. and 16u + ..; f takes r & 15 only, so
//   both hit the same sixteen distinct slots.
//
// Softmax: online, log2 domain. A wave compares against the row limits only
// on tiles that reach past its first row's limit; there a masked score
// becomes -inf and its p 0 by select. Dead rows of a live block run with
// q = 0 (finite scores) and are zeroed by select at the end. l sums the
// unrounded p per lane; the four lanes of a row are added in g order at the
// end. P is rounded to bf16 once, for P.V. The running max m is kept in one
// of two units, a compile-time trait of the step:
//   KtRawM   raw-score units: p = exp2(fma(s, c2, -m c2)), c2 = scale*log2e,
//            m_nat = m * scale (the bf16 caches)
//   KtLog2M  log2 units, for scores that already carry their scale:
//            p = exp2(s + -m), m_nat = m * ln2 (the e4m3 cache)
//
// Epilogue: num_splits == 1 normalises and writes bf16 rows as 16-byte
// stores (row layout: through an LDS image; key-split: straight from the
// fold); otherwise fp32 (m, l, o[D]) partials in the workspace layout of
// attn_decode_ragged_combine with rows = B*Tq*Hq, which
// tok_attn_ragged_combine folds in split order. No atomics, every sum in a
// fixed order; the grid depends on shapes alone: capturable, bitwise
// repeatable, slot-independent.
//
// kt_attn<D, R, KEYSPLIT, Src> is the bf16 kernel. Src alone knows the cache
// format: it is built from the kernel arguments, names Tmax, issues the DMAs
// of tile t into an LDS address, and keeps whatever it prefetches between
// tiles. The __global__ entries stay in the .hip files with their argument
// lists, so a kernel's argument segment is what its format needs.
#pragma once

#include <type_traits>

#include "common.h"

// KT_KERNEL marks a kernel, KT_SEG a segment of one. Both carry the same
// target attribute: the HIP headers' __shfl / __shfl_xor do not, so the
// compiler keeps them out of line in either (a callee with other target
// features is not inlined), as it did when this code stood in the kernels
// themselves. Making the shuffles inline is a speed change of its own and is
// left to one.
#if defined(__HIP_DEVICE_COMPILE__)
#define KT_KERNEL __global__ __attribute__((target("no-packed-fp32-ops")))
#define KT_SEG DEVINL __attribute__((target("no-packed-fp32-ops")))
#else
#define KT_KERNEL __global__
#define KT_SEG DEVINL
#endif

using bf16x8v = __attribute__((ext_vector_type(8))) __bf16;
using bf16x2v = __attribute__((ext_vector_type(2))) __bf16;
using i16x4v = __attribute__((ext_vector_type(4))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;

constexpr int KT_NTH = 256;
constexpr int KT_PAGE = 64;  // keys per tile = tokens per page
constexpr float KT_LOG2E = 1.4426950408889634f;
constexpr float KT_LN2 = 0.6931471805599453f;

// ---- primitives ----------------------------------------------------------

typedef __attribute__((address_space(3))) i16x4v* kt_tr_ptr;

DEVINL i16x4v kt_tr_read(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((kt_tr_ptr)p);
}

// 16 bytes per lane, global -> LDS: lane i's bytes land at lds_dst + 16 i.
DEVINL void kt_glds16(uint32_t voff, const void* sbase, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_dst)
      : "memory");
}

// 4 bytes per lane: lane i's dword lands at lds_dst + 4 i.
DEVINL void kt_glds4(uint32_t voff, const void* sbase, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
      "global_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_dst)
      : "memory");
}

DEVINL void kt_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// chunk swizzle f of the bf16 image
template <int D>
DEVINL int kt_swz(int r) {
  if (D == 128)
    return ((r & 3) << 2) | (((r >> 2) & 1) << 1) | ((r >> 3) & 1);
  return (((r >> 1) & 1) << 2) | (((r >> 2) & 1) << 1) | ((r >> 3) & 1);
}

DEVINL uint32_t kt_pack(float lo, float hi) {
  const f32x2 f = {lo, hi};
  union { bf16x2v b; uint32_t u; } c;
  c.b = __builtin_convertvector(f, bf16x2v);
  return c.u;
}

// packed row (token i, head r of the group) = i*R + r -> index in [B*Tq*Hq]
template <int R>
struct KtRows {
  long tok0;   // b * Tq
  int Hq, h0;  // h0 = hkv * R
  DEVINL long global(int row) const {
    return (tok0 + row / R) * Hq + h0 + row % R;
  }
};

// A wave-uniform pointer, pinned to SGPRs for the DMA's scalar base.
DEVINL const char* kt_uniform(const char* p) {
  const uint64_t a = (uint64_t)(uintptr_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  return (const char*)(uintptr_t)(((uint64_t)hi << 32) | lo);
}

// ---- the units of the running max ----------------------------------------

struct KtRawM {
  float c2, scale;  // c2 = scale * log2e
  KT_SEG float neg(float m_new) const { return -m_new * c2; }
  KT_SEG float ex(float s, float neg_m) const {
    return __builtin_amdgcn_exp2f(__builtin_fmaf(s, c2, neg_m));
  }
  KT_SEG float fold(float mw, float M) const {
    return __builtin_amdgcn_exp2f((mw - M) * c2);
  }
  KT_SEG float nat(float m) const { return m * scale; }
};

struct KtLog2M {
  KT_SEG float neg(float m_new) const { return -m_new; }
  KT_SEG float ex(float s, float neg_m) const {
    return __builtin_amdgcn_exp2f(s + neg_m);
  }
  KT_SEG float fold(float mw, float M) const {
    return __builtin_amdgcn_exp2f(mw - M);
  }
  KT_SEG float nat(float m) const { return m * KT_LN2; }
};

// ---- geometry --------------------------------------------------------------

// What is uniform over the block.
template <int D, int R, bool KEYSPLIT>
struct KtBlock {
  static constexpr int BM = KEYSPLIT ? 16 : 64;  // packed q rows per block
  int tid, lane, wid, li, lg, hkv, b, sp, S, NR;
  int m, base_pos, row_blk, i_first, kbeg, kend;
  KtRows<R> rows;
  long ws_ml0;

  KT_SEG KtBlock(const int* lens, const int* qlens, int Tq, int Tmax, int Hkv,
                 int MT, int chunk) {
    tid = threadIdx.x;
    lane = tid & 63;
    wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    li = lane & 15, lg = lane >> 4;
    hkv = blockIdx.x / MT;
    const int mt = blockIdx.x - hkv * MT;
    b = blockIdx.y, sp = blockIdx.z;
    S = gridDim.z;
    const int Hq = Hkv * R;
    NR = Tq * R;                               // packed rows of this kv head

    const int n = min(max(lens[b], 0), Tmax);
    m = min(max(qlens[b], 0), min(Tq, n));
    base_pos = n - m;                          // position of query 0

    row_blk = mt * BM;
    i_first = row_blk / R;
    const int i_last = min(m - 1, (row_blk + BM - 1) / R);
    const int p_last = base_pos + i_last;
    kbeg = sp * chunk;
    kend = min(kbeg + chunk, p_last + 1);

    rows = KtRows<R>{(long)b * Tq, Hq, hkv * R};
    ws_ml0 = (long)gridDim.y * Tq * Hq * S * D;  // the (m, l) pairs follow o
  }
  // block-uniform: nothing to attend to
  KT_SEG bool dead() const { return i_first >= m || kbeg >= kend; }
  KT_SEG int ntiles() const { return (kend - kbeg + KT_PAGE - 1) / KT_PAGE; }
};

// What is uniform over a wave, and the lane's score row.
struct KtWave {
  int row_w, kt0;        // wave's first row and first 16-key group
  bool wave_live, live_s;
  int lim_first, lim_last, row_s, lim_s;

  template <int D, int R, bool KEYSPLIT>
  KT_SEG explicit KtWave(const KtBlock<D, R, KEYSPLIT>& g) {
    row_w = g.row_blk + (KEYSPLIT ? 0 : g.wid * 16);
    kt0 = KEYSPLIT ? g.wid : 0;
    wave_live = row_w < g.NR && row_w / R < g.m;       // wave-uniform
    lim_first = g.base_pos + row_w / R;
    lim_last = g.base_pos + min(g.m - 1, (row_w + 15) / R);
    row_s = row_w + g.li;                              // the lane's score row
    live_s = row_s < g.NR && row_s / R < g.m;
    lim_s = live_s ? g.base_pos + row_s / R : -1;
  }
};

// Fragment read offsets, bytes within a bf16 tile.
template <int D, bool KEYSPLIT>
struct KtFrag {
  uint32_t k_off[D / 32];  // + kt * 16 * RB
  // transposed read: lane 4q+p of group g supplies row 16u + 4g + q, columns
  // 16dt + 4p .. + 3: chunk 2dt + (p >> 1), half p & 1. Row layout: u = 0, 1
  // (+ 32kk); key-split: u = w only.
  uint32_t v_base[2], v_x[2];

  KT_SEG KtFrag(int lane, int wid) {
    constexpr int RB = D * 2;
    const int li = lane & 15, lg = lane >> 4;
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks)
      k_off[ks] = li * RB + 16 * ((4 * ks + lg) ^ kt_swz<D>(li));
    const int tq = (lane >> 2) & 3, tp = lane & 3;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = 16 * (KEYSPLIT ? wid : u) + 4 * lg + tq;
      v_base[u] = r * RB + 8 * (tp & 1);
      v_x[u] = (tp >> 1) ^ kt_swz<D>(r & 15);
    }
  }
};

// ---- segments ------------------------------------------------------------

// A dead block's output: zero rows, or zero partials with m = -inf, l = 0.
template <int D, int R, bool KEYSPLIT>
KT_SEG void kt_write_dead(const KtBlock<D, R, KEYSPLIT>& g, bf16_t* out,
                          float* ws) {
  constexpr int CPR = D / 8;
  const int S = g.S, sp = g.sp;
  for (int idx = g.tid; idx < g.BM * CPR; idx += KT_NTH) {
    const int row = g.row_blk + idx / CPR, ch = idx % CPR;
    if (row >= g.NR) continue;
    const long gr = g.rows.global(row);
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
        ws[g.ws_ml0 + (gr * S + sp) * 2] = -INFINITY;
        ws[g.ws_ml0 + (gr * S + sp) * 2 + 1] = 0.f;
      }
    }
  }
}

// Q as the B operand of S^T, resident. A dead row loads nothing: zeros.
template <int D, int R, bool KEYSPLIT>
KT_SEG void kt_load_q(bf16x8v (&qf)[D / 32], const bf16_t* q,
                      const KtBlock<D, R, KEYSPLIT>& g, const KtWave& w) {
  const bf16_t* qrow =
      q + g.rows.global(w.live_s ? w.row_s : g.row_blk) * D + g.lg * 8;
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) {
    uint4 raw = {0, 0, 0, 0};
    if (w.live_s) raw = *reinterpret_cast<const uint4*>(qrow + ks * 32);
    union { uint4 u; bf16x8v f; } c;
    c.u = raw;
    qf[ks] = c.f;
  }
}

// Use q before the loop, so that the compiler's wait for the q loads sits
// there (tile 0 must land anyway) and not as a vmcnt(0) inside the loop.
template <int KS>
KT_SEG void kt_pin_q(bf16x8v (&qf)[KS]) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks]));
}

// S^T = K Q^T from a bf16 image: st[kt][j] = score of (key 16kt + 4g + j of
// the rows at kt_lds, q row li).
template <int D, int NKT>
KT_SEG void kt_scores(f32x4 (&st)[NKT], const char* kt_lds,
                      const uint32_t (&k_off)[D / 32],
                      const bf16x8v (&qf)[D / 32]) {
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    st[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks) {
      union { uint4 u; bf16x8v f; } a;
      a.u = *reinterpret_cast<const uint4*>(kt_lds + kt * 16 * (D * 2) +
                                            k_off[ks]);
      st[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.f, qf[ks], st[kt], 0,
                                                       0, 0);
    }
  }
}

// One tile of the online softmax on the scores of keys kw0 + 16kt + 4g + j:
// mask, max, p = exp2, l and m updated; st holds the unrounded p on return.
// Returns alpha, the rescale of what the row has accumulated so far.
template <int NKT, class MU>
KT_SEG float kt_softmax_step(f32x4 (&st)[NKT], float& m_run, float& l_run,
                             const MU& mu, int kw0, int lg, const KtWave& w) {
  const bool needs_mask = kw0 + 16 * NKT - 1 > w.lim_first;  // wave-uniform
  if (needs_mask) {
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        st[kt][j] = (kw0 + 16 * kt + 4 * lg + j <= w.lim_s) ? st[kt][j]
                                                            : -INFINITY;
  }

  float tmax = st[0][0];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int j = 0; j < 4; ++j) tmax = fmaxf(tmax, st[kt][j]);
  tmax = fmaxf(tmax, __shfl_xor(tmax, 16, WAVE));
  tmax = fmaxf(tmax, __shfl_xor(tmax, 32, WAVE));
  const float m_new = fmaxf(m_run, tmax);
  // a row with no key yet keeps m = -inf; its exponent offset is 0, so
  // that exp2(-inf + 0) is 0 and never exp2(-inf + inf)
  const float neg_m = (m_new == -INFINITY) ? 0.f : mu.neg(m_new);
  const float alpha = mu.ex(m_run, neg_m);
  m_run = m_new;

  float psum = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float p = mu.ex(st[kt][j], neg_m);
      if (needs_mask) p = (kw0 + 16 * kt + 4 * lg + j <= w.lim_s) ? p : 0.f;
      st[kt][j] = p;
      psum += p;
    }
  l_run = __builtin_fmaf(l_run, alpha, psum);
  return alpha;
}

// o_acc *= alpha: alpha of output row 4g + j lives in lane 4g + j
template <int DT>
KT_SEG void kt_rescale(f32x4 (&o_acc)[DT], float alpha, int lg) {
  float al[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) al[j] = __shfl(alpha, 4 * lg + j, WAVE);
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int j = 0; j < 4; ++j) o_acc[dt][j] *= al[j];
}

// O += P V on the wave's 16 keys (NKT = 1): P IS the A operand of the K = 16
// MFMA; vt is the V image, v_base / v_x the lane's transposed-read offsets.
template <int D>
KT_SEG void kt_pv16(f32x4 (&o_acc)[D / 16], const f32x4& p, const char* vt,
                    uint32_t v_base, uint32_t v_x) {
  union { uint32_t w[2]; i16x4v f; } pa;
  pa.w[0] = kt_pack(p[0], p[1]);
  pa.w[1] = kt_pack(p[2], p[3]);
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) {
    const i16x4v vb = kt_tr_read(vt + v_base + 16 * ((2 * dt) ^ v_x));
    o_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(pa.f, vb, o_acc[dt],
                                                          0, 0, 0);
  }
}

// O += P V on the 64 keys of a tile (NKT = 4): one rounding of P to bf16.
template <int D>
KT_SEG void kt_pv64(f32x4 (&o_acc)[D / 16], const f32x4 (&st)[4],
                    const char* vt, const uint32_t (&v_base)[2],
                    const uint32_t (&v_x)[2]) {
  bf16x8v pa[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    union { uint32_t w[4]; bf16x8v f; } c;
    c.w[0] = kt_pack(st[2 * kk][0], st[2 * kk][1]);
    c.w[1] = kt_pack(st[2 * kk][2], st[2 * kk][3]);
    c.w[2] = kt_pack(st[2 * kk + 1][0], st[2 * kk + 1][1]);
    c.w[3] = kt_pack(st[2 * kk + 1][2], st[2 * kk + 1][3]);
    pa[kk] = c.f;
  }
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
      union { i16x4v s[2]; bf16x8v f; } vb;
#pragma unroll
      for (int u = 0; u < 2; ++u)
        vb.s[u] = kt_tr_read(vt + kk * 32 * (D * 2) + v_base[u] +
                             16 * ((2 * dt) ^ v_x[u]));
      o_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa[kk], vb.f,
                                                          o_acc[dt], 0, 0, 0);
    }
}

// Key-split: the four waves' states of the 16 rows through the fp32 image at
// smem, folded in wave order by 16 * D/8 threads and written out.
template <int D, int R, class MU>
KT_SEG void kt_fold_store(char* smem, const f32x4 (&o_acc)[D / 16],
                          float m_run, float l_row,
                          const KtBlock<D, R, true>& g, const MU& mu,
                          bf16_t* out, float* ws) {
  constexpr int CPR = D / 8, DT = D / 16;
  constexpr int FLD = D + 2;                   // fp32 fold row: o[D], m, l
  const int S = g.S, sp = g.sp, li = g.li, lg = g.lg;
  float* img = reinterpret_cast<float*>(smem);
  float* mine = img + g.wid * 16 * FLD;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
      mine[(4 * lg + j) * FLD + dt * 16 + li] = o_acc[dt][j];
  if (lg == 0) {
    mine[li * FLD + D] = m_run;
    mine[li * FLD + D + 1] = l_row;
  }
  __syncthreads();
  const int r = g.tid / CPR, ch = g.tid % CPR;
  if (g.tid < 16 * CPR && r < g.NR) {
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) M = fmaxf(M, img[(w * 16 + r) * FLD + D]);
    float L = 0.f, acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float* src = img + (w * 16 + r) * FLD;
      const float mw = src[D];
      const float e = (mw == -INFINITY) ? 0.f : mu.fold(mw, M);
      L = __builtin_fmaf(src[D + 1], e, L);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        acc[j] = __builtin_fmaf(src[ch * 8 + j], e, acc[j]);
    }
    const long gr = g.rows.global(r);
    if (S == 1) {
      const float inv = (L > 0.f) ? 1.f / L : 0.f;
      bf16x8 o8;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o8.h[j] = f2bfbits((inv > 0.f) ? acc[j] * inv : 0.f);
      *reinterpret_cast<bf16x8*>(out + gr * D + ch * 8) = o8;
    } else {
      float* po = ws + (gr * S + sp) * D + ch * 8;
      f32x4v lo, hi;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        lo.v[j] = (L > 0.f) ? acc[j] : 0.f;
        hi.v[j] = (L > 0.f) ? acc[4 + j] : 0.f;
      }
      reinterpret_cast<f32x4v*>(po)[0] = lo;
      reinterpret_cast<f32x4v*>(po)[1] = hi;
      if (ch == 0) {
        ws[g.ws_ml0 + (gr * S + sp) * 2] =
            (M == -INFINITY) ? -INFINITY : mu.nat(M);
        ws[g.ws_ml0 + (gr * S + sp) * 2 + 1] = L;
      }
    }
  }
}

// Row layout, one split: normalised bf16 rows through the image at smem.
template <int D, int R>
KT_SEG void kt_store_rows(char* smem, const f32x4 (&o_acc)[D / 16],
                          float l_row, const KtBlock<D, R, false>& g,
                          const KtWave& w, bf16_t* out) {
  constexpr int CPR = D / 8, DT = D / 16;
  constexpr int OLD = D + 8;                   // epilogue row, bf16 elements
  const int li = g.li, lg = g.lg;
  const float inv = (l_row > 0.f) ? 1.f / l_row : 0.f;
  bf16_t* img = reinterpret_cast<bf16_t*>(smem) + g.wid * 16 * OLD;
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
    const int idx = it * WAVE + g.lane;
    const int r = idx / CPR, ch = idx % CPR;
    const int row = w.row_w + r;
    if (row < g.NR)
      *reinterpret_cast<uint4*>(out + g.rows.global(row) * D + ch * 8) =
          *reinterpret_cast<const uint4*>(img + r * OLD + ch * 8);
  }
}

// Row layout, several splits: the partial (m in natural-log units, l,
// unnormalised o).
template <int D, int R, class MU>
KT_SEG void kt_store_partials(const f32x4 (&o_acc)[D / 16], float m_run,
                              float l_row, const KtBlock<D, R, false>& g,
                              const KtWave& w, const MU& mu, float* ws) {
  const int S = g.S, sp = g.sp, li = g.li, lg = g.lg;
  const float m_nat = (m_run == -INFINITY) ? -INFINITY : mu.nat(m_run);
  if (lg == 0 && w.row_s < g.NR) {
    const long gr = g.rows.global(w.row_s);
    ws[g.ws_ml0 + (gr * S + sp) * 2] = m_nat;
    ws[g.ws_ml0 + (gr * S + sp) * 2 + 1] = l_row;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float lj = __shfl(l_row, 4 * lg + j, WAVE);
    const int row = w.row_w + 4 * lg + j;
    if (row < g.NR) {
      float* po = ws + (g.rows.global(row) * S + sp) * D + li;
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt)
        po[dt * 16] = (lj > 0.f) ? o_acc[dt][j] : 0.f;
    }
  }
}

// After the key loop: drain the DMAs nobody reads, sum l over the four lanes
// of a row in g order, and write the block's result in its layout. smem must
// hold 4 * 16 * (D + 2) floats.
template <int D, int R, bool KEYSPLIT, class MU>
KT_SEG void kt_finish(char* smem, const f32x4 (&o_acc)[D / 16], float m_run,
                      float l_run, const KtBlock<D, R, KEYSPLIT>& g,
                      const KtWave& w, const MU& mu, bf16_t* out, float* ws) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  kt_barrier();

  float l_row = 0.f;
#pragma unroll
  for (int gg = 0; gg < 4; ++gg) l_row += __shfl(l_run, g.li + 16 * gg, WAVE);
  if (!w.live_s || !w.wave_live) {   // dead rows: no state, by select
    l_row = 0.f;
    m_run = -INFINITY;
  }

  if constexpr (KEYSPLIT)
    kt_fold_store<D, R>(smem, o_acc, m_run, l_row, g, mu, out, ws);
  else if (g.S == 1)
    kt_store_rows<D, R>(smem, o_acc, l_row, g, w, out);
  else
    kt_store_partials<D, R>(o_acc, m_run, l_row, g, w, mu, ws);
}

// ---- the bf16 kernel -------------------------------------------------------

// Src: Tmax(), begin(block, Hkv, d_row, d_ch), issue(tile, lds_dst) for the
// 2 * NJ DMAs of the K and V tile (rows past kend - 1 clamped), and
// prefetch(tile) for whatever it reads ahead of the issue of that tile.
template <int D, int R, bool KEYSPLIT, class Src>
KT_SEG void kt_attn(Src src, const bf16_t* q, const int* lens,
                    const int* qlens, bf16_t* out, float* ws, int Tq, int Hkv,
                    int MT, int chunk, float scale) {
  constexpr int RB = D * 2;                    // bytes per tile row
  constexpr int TILE = KT_PAGE * RB;           // one K or V tile
  constexpr int NJ = TILE / 4096;              // DMA instructions per tile
  constexpr int CPR = D / 8;                   // 16-byte chunks per row
  constexpr int KS = D / 32;                   // k steps of S^T
  constexpr int DT = D / 16;                   // d tiles of O
  constexpr int NKT = KEYSPLIT ? 1 : 4;        // 16-key groups per wave
  __shared__ __attribute__((aligned(1024))) char smem[4 * TILE];
  static_assert(4 * 16 * (D + 8) * 2 <= 4 * TILE, "epilogue image fits");
  static_assert(4 * 16 * (D + 2) * 4 <= 4 * TILE, "fold image fits");

  const KtBlock<D, R, KEYSPLIT> g(lens, qlens, Tq, src.Tmax(), Hkv, MT, chunk);
  if (g.dead()) {
    kt_write_dead(g, out, ws);
    return;
  }
  const KtWave w(g);

  bf16x8v qf[KS];
  kt_load_q(qf, q, g, w);

  // ---- DMA geometry ----
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane(
      (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem +
      g.wid * 1024);
  const int d_row = g.tid / CPR;                       // row within 4 KiB
  const int d_ch = (g.tid % CPR) ^ kt_swz<D>(d_row & 15);
  const int ntiles = g.ntiles();
  const KtFrag<D, KEYSPLIT> fr(g.lane, g.wid);

  const KtRawM mu{scale * KT_LOG2E, scale};
  float m_run = -INFINITY, l_run = 0.f;
  f32x4 o_acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o_acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  src.begin(g.b, g.hkv, Hkv, g.kbeg, g.kend, d_row, d_ch);
  src.issue(0, lds0);
  src.prefetch(min(1, ntiles - 1));
  kt_pin_q(qf);
  for (int t = 0; t < ntiles; ++t) {
    const int buf = t & 1;
    src.issue(min(t + 1, ntiles - 1), lds0 + (buf ^ 1) * 2 * TILE);
    src.prefetch(min(t + 2, ntiles - 1));
    if (NJ == 4)
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    kt_barrier();

    const int kw0 = g.kbeg + t * KT_PAGE + 16 * w.kt0;  // wave's first key
    if (w.wave_live && kw0 <= w.lim_last) {
      const char* kt_lds = smem + buf * 2 * TILE + w.kt0 * 16 * RB;
      const char* vt_lds = smem + buf * 2 * TILE + TILE;

      f32x4 st[NKT];
      kt_scores<D>(st, kt_lds, fr.k_off, qf);
      const float alpha = kt_softmax_step(st, m_run, l_run, mu, kw0, g.lg, w);
      kt_rescale(o_acc, alpha, g.lg);
      if constexpr (KEYSPLIT)
        kt_pv16<D>(o_acc, st[0], vt_lds, fr.v_base[0], fr.v_x[0]);
      else
        kt_pv64<D>(o_acc, st, vt_lds, fr.v_base, fr.v_x);
    }
    kt_barrier();
  }
  kt_finish(smem, o_acc, m_run, l_run, g, w, mu, out, ws);
}

// f(std::integral_constant<int, D>, std::integral_constant<int, R>) for the
// head sizes and group sizes the kernels are built for; false for any other.
template <class F>
bool kt_dispatch(int D, int R, F&& f) {
  auto by_r = [&](auto d) {
    switch (R) {
      case 1: f(d, std::integral_constant<int, 1>{}); return true;
      case 2: f(d, std::integral_constant<int, 2>{}); return true;
      case 4: f(d, std::integral_constant<int, 4>{}); return true;
      case 8: f(d, std::integral_constant<int, 8>{}); return true;
      default: return false;
    }
  };
  if (D == 128) return by_r(std::integral_constant<int, 128>{});
  if (D == 64) return by_r(std::integral_constant<int, 64>{});
  return false;
}

// ---- appends ---------------------------------------------------------------

// Where token position p of sequence b goes: the cache row (an index into
// [rows, D] and into the scales [rows]) of kv head h, or -1 for a dead token.
struct KtContigDest {  // cache [B,Tmax,Hkv,D]
  int Tmax, Hkv;
  KT_SEG long row(int b, long p, bool live, int h) const {
    if (!live || p < 0 || p >= Tmax) return -1;
    return ((long)b * Tmax + p) * Hkv + h;
  }
};

struct KtPagedDest {  // pool [P,Hkv,64,D], page_table [B,NP]
  const int* page_table;
  int NP, P, Hkv;
  // The table is read only at an index inside it; an id outside [0, P) is a
  // dead token (a clamped write would land in someone else's page).
  KT_SEG long row(int b, long p, bool live, int h) const {
    if (!live || p < 0 || p >= (long)NP * KT_PAGE) return -1;
    const int pid = page_table[(long)b * NP + p / KT_PAGE];
    if (pid < 0 || pid >= P) return -1;
    return ((long)pid * Hkv + h) * KT_PAGE + p % KT_PAGE;
  }
};

inline int kt_append_grid(long nwork) {
  long grid = (nwork + KT_NTH - 1) / KT_NTH;
  if (grid > 8192) grid = 8192;
  if (grid < 1) grid = 1;
  return (int)grid;
}
