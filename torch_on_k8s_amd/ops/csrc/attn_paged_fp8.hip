// FP8 (OCP e4m3) paged KV cache on MI355X (gfx950): MFMA attention over e4m3
// pages for decode (Tq = 1) and chunked prefill (Tq > 1), and the two appends
// that write tokens into their pages.
//
// Format. kpool/vpool [P,Hkv,64,D] e4m3 codes: one (page, kv head) is a
// contiguous slab of 64*D bytes. kscale/vscale [P,Hkv,64] fp32: one scale per
// (page, head, slot), a contiguous 256-byte strip per slab. An element means
// float(code) * scale; the quantizer is that of kv_fp8.hip
// (ops.quantize_rows_fp8), a function of the bf16 row the bf16 kernels would
// have stored. page_table [B,NP] int32, lens/qlens [B] int32 and the page size
// are those of attn_paged.hip.
//
//   attn_paged_fp8_kernel<D, R, KEYSPLIT>  grid (Hkv * row_tiles, B, splits)
//     The contract of attn_paged_kernel, taken unchanged: grid, (lens, qlens,
//     page_table), page ids clamped into [0, P), the split workspace and the
//     tok_attn_ragged_combine fold, zero rows for i >= m, the row layout and
//     the key-split layout with their switch at Tq * R <= 16. q and P stay
//     bf16 and the accumulators fp32; an e4m3 code is exactly a bf16 value, so
//     both products run on the bf16 MFMAs over the CODES and the two row
//     scales are folded in outside them:
//       score = acc * (kscale[key] * softmax_scale * log2e)   once per key,
//               before the max: the softmax runs in the log2 domain on it
//       P     = bf16(p * vscale[key])   one fp32 product, then P's single
//               rounding to bf16; l sums the unscaled, unrounded p
//     A row with scale 0 scores 0 and contributes p * 0.
//
// Staging. A key tile is a page. Per tile every wave issues the same 2 NJ + 2
// DMAs (NJ = 64 D / 4096: 2 at D = 128, 1 at D = 64): its 1 KiB share of each
// 4 KiB of the K and of the V code slab by 16-byte global_load_lds_dwordx4
// (inline asm, M0 saved and restored), and the two 256-byte scale strips by
// global_load_lds_dword into a strip pair of ITS OWN (4 x 512 bytes per
// buffer): a wave reads scales only from what it loaded itself. Two buffers;
// tile t + 1 is issued, one counted vmcnt(2 NJ + 2) says tile t has landed in
// this wave, a barrier says so of every wave, a last barrier frees the
// buffer. The page id of tile t + 2 is a scalar load one tile ahead. The
// source slot is min(slot, last valid slot of the tile) for the codes AND for
// the scales, so a NaN code or a NaN scale in a row >= n of a tail page, or
// anything in an unreferenced page, never enters LDS. The DMA targets lie in
// the first 36 KiB of LDS (M0 carries a 16-bit address).
//
// Codes image. Rows of D bytes, D/16 chunks of 16 bytes; chunk c of row r
// sits at chunk c ^ g(r), g(r) = (r >> 1) & 7 at D = 128 and (r >> 2) & 3 at
// D = 64. Bank argument: the key-split K read is a b64 of lane (i, g) at row
// 16w + i, chunk 2ks + (g >> 1), half g & 1; a b64 is served 32 lanes at a
// time (g = 0, 1: one chunk of sixteen rows). Sixteen rows cover 16 D bytes,
// a multiple of the 256 bytes the 64 banks span, and within 256 bytes row r
// starts at (r & 1) * 128 (D = 128) or (r & 3) * 64 (D = 64); g spreads the
// rows that share a start over all chunk positions, so the sixteen 16-byte
// slots are distinct: no conflict. The widening reads below are b128 over
// consecutive chunks of consecutive rows: a permutation of a linear 1 KiB.
//
// Widening. v_cvt_scalef32_pk_bf16_fp8 at scale 1.0: one instruction per two
// codes. Wave w owns rows 16w .. 16w + 15 of the K and of the V slab of every
// tile in both layouts; no code is widened twice in a block.
//   Key-split (Tq * R <= 16, decode): a wave only consumes its own 16 keys.
//     K fragments come straight from the codes image (8 codes per lane and
//     k-step, widened in registers, A operand of mfma_f32_16x16x32_bf16). V
//     rows are widened into the wave's 16 x D bf16 strip (rows 16w.. of a
//     64-row image with the swizzle of attn_paged.hip) and read back by
//     ds_read_b64_tr_b16 under the map of attn_paged.hip for
//     mfma_f32_16x16x16_bf16. Producer and consumer are the same wave: an
//     lgkmcnt(0), no block barrier.
//   Row layout (chunked prefill): each wave widens its 16 K and 16 V rows
//     into the bf16 image of attn_paged.hip (same swizzle, same fragment
//     reads), one more barrier per tile.
//   The halved tile bytes go to blocks per CU, not to a third buffer: LDS is
//   what bounds occupancy here (52 KiB key-split and 68 KiB row layout at
//   D = 128 against 64 KiB of the bf16 kernel), and a decode grid of
//   Hkv * B * splits blocks hides latency with resident blocks.
//
// Resources (hipcc -O3 --offload-arch=gfx950,
// -Rpass-analysis=kernel-resource-usage; scratch is 0 B everywhere):
//   kernel                                    VGPR  AGPR  SGPR  LDS B  waves/SIMD
//   attn_paged_fp8_kernel<128,1,true>           104     0    66  53248  3
//   attn_paged_fp8_kernel<128,2|4|8,true>       104     0    69  53248  3
//   attn_paged_fp8_kernel<128,1,false>          180     0    67  69632  2
//   attn_paged_fp8_kernel<128,2|4|8,false>      180     0    72  69632  2
//   attn_paged_fp8_kernel<64,1,true>             68     0    65  28672  5
//   attn_paged_fp8_kernel<64,2|4|8,true>         68     0    68  28672  5
//   attn_paged_fp8_kernel<64,1,false>           130     0    66  36864  3
//   attn_paged_fp8_kernel<64,2|4|8,false>       130     0    71  36864  3
//   qkv_rope_append_paged_fp8_kernel<8|4>        60     0    64      0  8
//   kv_quantize_append_paged_kernel<16|8>     29|28     0    60      0  8
// (waves/SIMD as the compiler reports it; LDS bounds it in the key-split
// layout, three blocks per CU at D = 128 where the bf16 kernel has two; the
// row layout keeps two, with the codes of 16 K and 16 V rows in registers on
// their way to the image.) In the .s every tile loop holds exactly one
// s_waitcnt vmcnt(6) (vmcnt(4) at D = 64) in front of its first barrier and no
// vmcnt(0). The widening that shipped is v_cvt_scalef32_pk_bf16_fp8: exact on
// the hardware for every non-NaN code (tests/test_attention_paged_fp8_gpu.py,
// random codes over all byte values against fp64).
//
//   qkv_rope_append_paged_fp8_kernel / kv_quantize_append_paged_kernel
//     qkv_rope_append_fp8_kernel and kv_quantize_append_kernel of kv_fp8.hip
//     with the destination looked up in the table as
//     qkv_rope_append_paged_kernel does: the same arithmetic per element, so
//     the same codes and scale for the same token. A token is dead if
//     i >= qlens[b], its position is outside [0, 64 NP) or its table entry is
//     outside [0, P); it writes neither codes nor scale and gets a zero q row.
#include "common.h"

extern "C" hipError_t tok_attn_ragged_combine(const float* ws, void* out,
                                              int rows, int Hq, int D,
                                              int num_splits,
                                              hipStream_t stream);

namespace {

#if defined(__HIP_DEVICE_COMPILE__)
#define PF_KERNEL __global__ __attribute__((target("no-packed-fp32-ops")))
#else
#define PF_KERNEL __global__
#endif

using bf16x8v = __attribute__((ext_vector_type(8))) __bf16;
using bf16x2v = __attribute__((ext_vector_type(2))) __bf16;
using i16x4v = __attribute__((ext_vector_type(4))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;

constexpr int PF_NTH = 256;
constexpr int PF_PAGE = 64;  // tokens per page = keys per tile
constexpr float PF_LOG2E = 1.4426950408889634f;
constexpr float PF_LN2 = 0.6931471805599453f;
constexpr float PF_MAX = 448.f;

typedef __attribute__((address_space(3))) i16x4v* pf_tr_ptr;

DEVINL i16x4v pf_tr_read(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((pf_tr_ptr)p);
}

// 16 bytes per lane, global -> LDS: lane i's bytes land at lds_dst + 16 i.
DEVINL void pf_glds16(uint32_t voff, const void* sbase, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_dst)
      : "memory");
}

// 4 bytes per lane: lane i's dword lands at lds_dst + 4 i.
DEVINL void pf_glds4(uint32_t voff, const void* sbase, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
      "global_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_dst)
      : "memory");
}

DEVINL void pf_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// chunk swizzle of the bf16 image (attn_paged.hip)
template <int D>
DEVINL int pf_swz(int r) {
  if (D == 128)
    return ((r & 3) << 2) | (((r >> 2) & 1) << 1) | ((r >> 3) & 1);
  return (((r >> 1) & 1) << 2) | (((r >> 2) & 1) << 1) | ((r >> 3) & 1);
}

// chunk swizzle of the codes image, r in [0, 16)
template <int D>
DEVINL int pf_cswz(int r) {
  return D == 128 ? (r >> 1) & 7 : (r >> 2) & 3;
}

DEVINL uint32_t pf_pack(float lo, float hi) {
  const f32x2 f = {lo, hi};
  union { bf16x2v b; uint32_t u; } c;
  c.b = __builtin_convertvector(f, bf16x2v);
  return c.u;
}

// two e4m3 codes (the low or the high half of w) -> two bf16, exactly
template <bool HI>
DEVINL uint32_t pf_widen2(uint32_t w) {
  union { bf16x2v b; uint32_t u; } c;
  c.b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI);
  return c.u;
}

// 16 rows of the codes image -> the same 16 rows of the bf16 image, by one
// wave; both pointers are at a row that is a multiple of 16.
template <int D>
DEVINL void pf_widen16(const char* codes, char* img, int lane) {
  constexpr int CPC = D / 16;  // chunks per codes row
#pragma unroll
  for (int it = 0; it < 16 * CPC / WAVE; ++it) {
    const int idx = it * WAVE + lane;
    const int row = idx / CPC, cc = idx % CPC;
    const uint4 raw = *reinterpret_cast<const uint4*>(
        codes + row * D + 16 * (cc ^ pf_cswz<D>(row)));
    const uint4 lo = {pf_widen2<false>(raw.x), pf_widen2<true>(raw.x),
                      pf_widen2<false>(raw.y), pf_widen2<true>(raw.y)};
    const uint4 hi = {pf_widen2<false>(raw.z), pf_widen2<true>(raw.z),
                      pf_widen2<false>(raw.w), pf_widen2<true>(raw.w)};
    char* dst = img + row * (D * 2);
    const int x = pf_swz<D>(row);
    *reinterpret_cast<uint4*>(dst + 16 * ((2 * cc) ^ x)) = lo;
    *reinterpret_cast<uint4*>(dst + 16 * ((2 * cc + 1) ^ x)) = hi;
  }
}

// packed row (token i, head r of the group) = i*R + r -> index in [B*Tq*Hq]
template <int R>
struct PfRows {
  long tok0;   // b * Tq
  int Hq, h0;  // h0 = hkv * R
  DEVINL long global(int row) const {
    return (tok0 + row / R) * Hq + h0 + row % R;
  }
};

// A wave-uniform pointer, pinned to SGPRs for the DMA's scalar base.
DEVINL const char* pf_uniform(const char* p) {
  const uint64_t a = (uint64_t)(uintptr_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  return (const char*)(uintptr_t)(((uint64_t)hi << 32) | lo);
}

struct PfPools {
  const char *k, *v, *ks, *vs;  // code pools and scale pools, as bytes
};

// Page raw_id (clamped into [0, P): never a fault) of kv head hkv, slots
// clamped to last_slot: this wave's share of the K and V code slabs to LDS
// address dst and the two scale strips to sdst. 2 NJ + 2 DMAs in every wave.
template <int D>
DEVINL void pf_stage(const PfPools& pools, int raw_id, int P, int Hkv, int hkv,
                     uint32_t dst, uint32_t sdst, int last_slot, int d_row,
                     int d_ch, int lane) {
  constexpr int CT = PF_PAGE * D, NJ = CT / 4096, RPS = 4096 / D;
  const long slab = (long)min(max(raw_id, 0), P - 1) * Hkv + hkv;
  const char* kb = pf_uniform(pools.k + slab * CT);
  const char* vb = pf_uniform(pools.v + slab * CT);
  const char* ksb = pf_uniform(pools.ks + slab * (PF_PAGE * 4));
  const char* vsb = pf_uniform(pools.vs + slab * (PF_PAGE * 4));
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int slot = min(j * RPS + d_row, last_slot);
    const uint32_t voff = (uint32_t)slot * D + d_ch * 16;
    pf_glds16(voff, kb, dst + j * 4096);
    pf_glds16(voff, vb, dst + CT + j * 4096);
  }
  const uint32_t soff = (uint32_t)min(lane, last_slot) * 4;
  pf_glds4(soff, ksb, sdst);
  pf_glds4(soff, vsb, sdst + PF_PAGE * 4);
}

template <int D, int R, bool KEYSPLIT>
PF_KERNEL __launch_bounds__(PF_NTH, 2) void attn_paged_fp8_kernel(
    const bf16_t* __restrict__ q, const uint8_t* __restrict__ kpool,
    const uint8_t* __restrict__ vpool, const float* __restrict__ kscale,
    const float* __restrict__ vscale, const int* __restrict__ page_table,
    const int* __restrict__ lens, const int* __restrict__ qlens,
    bf16_t* __restrict__ out, float* __restrict__ ws, int Tq, int NP, int P,
    int Hkv, int MT, int chunk, float scale) {
  constexpr int RB = D * 2;                    // bytes per bf16 image row
  constexpr int CT = PF_PAGE * D;              // one K or V code slab
  constexpr int NJ = CT / 4096;                // 16-byte DMAs per slab
  constexpr int CPC = D / 16;                  // 16-byte chunks per codes row
  constexpr int CPR = D / 8;                   // 16-byte chunks per bf16 row
  constexpr int SCB = 4 * 2 * PF_PAGE * 4;     // four waves' scale strip pairs
  constexpr int STAGE = 2 * CT + SCB;          // one staging buffer
  constexpr int IMG = (KEYSPLIT ? 1 : 2) * PF_PAGE * RB;  // bf16 image
  constexpr int KS = D / 32;                   // k steps of S^T
  constexpr int DT = D / 16;                   // d tiles of O
  constexpr int OLD = D + 8;                   // bf16 epilogue row, elements
  constexpr int FLD = D + 2;                   // fp32 fold row: o[D], m, l
  constexpr int BM = KEYSPLIT ? 16 : 64;       // packed q rows per block
  constexpr int NKT = KEYSPLIT ? 1 : 4;        // 16-key groups per wave
  constexpr int SMEM = 2 * STAGE + IMG;
  __shared__ __attribute__((aligned(1024))) char smem[SMEM];
  static_assert(2 * STAGE <= 65536, "DMA targets within 16 address bits");
  static_assert(4 * 16 * OLD * 2 <= SMEM, "epilogue image fits");
  static_assert(4 * 16 * FLD * 4 <= SMEM, "fold image fits");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int hkv = blockIdx.x / MT, mt = blockIdx.x - hkv * MT;
  const int b = blockIdx.y, sp = blockIdx.z;
  const int S = gridDim.z;
  const int Hq = Hkv * R;
  const int NR = Tq * R;                       // packed rows of this kv head
  const int Tmax = NP * PF_PAGE;

  const int n = min(max(lens[b], 0), Tmax);
  const int m = min(max(qlens[b], 0), min(Tq, n));
  const int base_pos = n - m;                  // position of query 0

  const int row_blk = mt * BM;
  const int i_first = row_blk / R;
  const int i_last = min(m - 1, (row_blk + BM - 1) / R);
  const int p_last = base_pos + i_last;
  const int kbeg = sp * chunk;
  const int kend = min(kbeg + chunk, p_last + 1);

  const PfRows<R> rows{(long)b * Tq, Hq, hkv * R};
  const long ws_ml0 = (long)gridDim.y * Tq * Hq * S * D;

  if (i_first >= m || kbeg >= kend) {  // block-uniform: nothing to attend to
    for (int idx = tid; idx < BM * CPR; idx += PF_NTH) {
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

  // ---- this wave's rows and keys ----
  const int row_w = row_blk + (KEYSPLIT ? 0 : wid * 16);  // wave's first row
  const int kt0 = KEYSPLIT ? wid : 0;          // wave's first 16-key group
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
  const uint32_t lds_base = __builtin_amdgcn_readfirstlane(
      (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem);
  const uint32_t lds0 = lds_base + wid * 1024;              // codes share
  const uint32_t sds0 = lds_base + 2 * CT + wid * (SCB / 4);  // scale strips
  const int d_row = tid / CPC;                         // slot within a 4 KiB
  const int d_ch = (tid % CPC) ^ pf_cswz<D>(d_row & 15);
  const PfPools pools{reinterpret_cast<const char*>(kpool),
                      reinterpret_cast<const char*>(vpool),
                      reinterpret_cast<const char*>(kscale),
                      reinterpret_cast<const char*>(vscale)};
  const int* tab = page_table + (long)b * NP;
  const int pg0 = kbeg / PF_PAGE;                      // < NP: kbeg < kend <= n
  const int ntiles = (kend - kbeg + PF_PAGE - 1) / PF_PAGE;
  const int krem = kend - 1 - kbeg;                    // last row, from kbeg

  // ---- fragment read offsets ----
  // key-split K: 8 codes of row 16w + li, bytes within a codes slab
  uint32_t kc_off[KS];
  // row layout K: bytes within a bf16 tile, + kt * 16 * RB
  uint32_t k_off[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    kc_off[ks] = (16 * wid + li) * D +
                 16 * ((2 * ks + (lg >> 1)) ^ pf_cswz<D>(li)) + 8 * (lg & 1);
    k_off[ks] = li * RB + 16 * ((4 * ks + lg) ^ pf_swz<D>(li));
  }
  // transposed read: lane 4q+p of group g supplies row 16u + 4g + q, columns
  // 16dt + 4p .. + 3: chunk 2dt + (p >> 1), half p & 1. Row layout: u = 0, 1
  // (+ 32kk); key-split: u = w only.
  uint32_t v_base[2], v_x[2];
  {
    const int tq = (lane >> 2) & 3, tp = lane & 3;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = 16 * (KEYSPLIT ? wid : u) + 4 * lg + tq;
      v_base[u] = r * RB + 8 * (tp & 1);
      v_x[u] = (tp >> 1) ^ pf_swz<D>(r & 15);
    }
  }
  char* const img = smem + 2 * STAGE;                  // bf16 image: K, then V
  char* const vimg = img + (KEYSPLIT ? 0 : PF_PAGE * RB);

  const float c2 = scale * PF_LOG2E;
  float m_run = -INFINITY, l_run = 0.f;                // m in log2 units
  f32x4 o_acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o_acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  pf_stage<D>(pools, tab[pg0], P, Hkv, hkv, lds0, sds0,
              min(PF_PAGE - 1, krem), d_row, d_ch, lane);
  int id_next = tab[pg0 + min(1, ntiles - 1)];         // raw id of tile t + 1
  // Use q here, so that the compiler's wait for the q loads sits before the
  // loop (tile 0 must land anyway) and not as a vmcnt(0) inside it.
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks]));
  for (int t = 0; t < ntiles; ++t) {
    const int buf = t & 1;
    pf_stage<D>(pools, id_next, P, Hkv, hkv, lds0 + (buf ^ 1) * STAGE,
                sds0 + (buf ^ 1) * STAGE,
                min(PF_PAGE - 1, krem - min(t + 1, ntiles - 1) * PF_PAGE),
                d_row, d_ch, lane);
    id_next = tab[pg0 + min(t + 2, ntiles - 1)];
    if (NJ == 2)
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    pf_barrier();

    const char* cbuf = smem + buf * STAGE;             // K codes, V codes
    const char* sbuf = cbuf + 2 * CT + wid * (SCB / 4);  // own kscale, vscale
    if constexpr (!KEYSPLIT) {
      pf_widen16<D>(cbuf + wid * 16 * D, img + wid * 16 * RB, lane);
      pf_widen16<D>(cbuf + CT + wid * 16 * D, vimg + wid * 16 * RB, lane);
      pf_barrier();
    }

    const int k0 = kbeg + t * PF_PAGE;
    const int kw0 = k0 + 16 * kt0;                     // wave's first key
    if (wave_live && kw0 <= lim_last) {
      if constexpr (KEYSPLIT)  // own 16 V rows -> own strip, read back below
        pf_widen16<D>(cbuf + CT + wid * 16 * D, vimg + wid * 16 * RB, lane);

      // S^T = K Q^T: st[kt][j] = score of (key kw0 + 16kt + 4g + j, row li)
      f32x4 st[NKT];
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        st[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          bf16x8v a;
          if constexpr (KEYSPLIT) {
            const uint2 raw =
                *reinterpret_cast<const uint2*>(cbuf + kc_off[ks]);
            union { uint32_t w[4]; bf16x8v f; } c;
            c.w[0] = pf_widen2<false>(raw.x);
            c.w[1] = pf_widen2<true>(raw.x);
            c.w[2] = pf_widen2<false>(raw.y);
            c.w[3] = pf_widen2<true>(raw.y);
            a = c.f;
          } else {
            union { uint4 u; bf16x8v f; } c;
            c.u = *reinterpret_cast<const uint4*>(img + kt * 16 * RB +
                                                  k_off[ks]);
            a = c.f;
          }
          st[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, qf[ks], st[kt],
                                                           0, 0, 0);
        }
      }

      // the row scales of the lane's keys 16(kt0 + kt) + 4g .. + 3
      f32x4 vsc[NKT];
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        const char* sp4 = sbuf + (16 * (kt0 + kt) + 4 * lg) * 4;
        const f32x4 ksc = *reinterpret_cast<const f32x4*>(sp4);
        vsc[kt] = *reinterpret_cast<const f32x4*>(sp4 + PF_PAGE * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) st[kt][j] *= ksc[j] * c2;
      }

      const bool needs_mask = kw0 + 16 * NKT - 1 > lim_first;  // wave-uniform
      if (needs_mask) {
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            st[kt][j] = (kw0 + 16 * kt + 4 * lg + j <= lim_s) ? st[kt][j]
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
      const float neg_m = (m_new == -INFINITY) ? 0.f : -m_new;
      const float alpha = __builtin_amdgcn_exp2f(m_run + neg_m);
      m_run = m_new;

      float psum = 0.f;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float p = __builtin_amdgcn_exp2f(st[kt][j] + neg_m);
          if (needs_mask)
            p = (kw0 + 16 * kt + 4 * lg + j <= lim_s) ? p : 0.f;
          psum += p;
          st[kt][j] = p * vsc[kt][j];   // vscale once, before P's rounding
        }
      l_run = __builtin_fmaf(l_run, alpha, psum);

      // alpha of output row 4g + j lives in lane 4g + j
      float al[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) al[j] = __shfl(alpha, 4 * lg + j, WAVE);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int j = 0; j < 4; ++j) o_acc[dt][j] *= al[j];

      if constexpr (KEYSPLIT) {
        // the strip this wave wrote above is in LDS before it is read
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // P of the wave's 16 keys IS the A operand of the K = 16 MFMA
        union { uint32_t w[2]; i16x4v f; } pa;
        pa.w[0] = pf_pack(st[0][0], st[0][1]);
        pa.w[1] = pf_pack(st[0][2], st[0][3]);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const i16x4v vb =
              pf_tr_read(vimg + v_base[0] + 16 * ((2 * dt) ^ v_x[0]));
          o_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(
              pa.f, vb, o_acc[dt], 0, 0, 0);
        }
      } else {
        // P as the A operand: one rounding to bf16
        bf16x8v pa[2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          union { uint32_t w[4]; bf16x8v f; } c;
          c.w[0] = pf_pack(st[2 * kk][0], st[2 * kk][1]);
          c.w[1] = pf_pack(st[2 * kk][2], st[2 * kk][3]);
          c.w[2] = pf_pack(st[2 * kk + 1][0], st[2 * kk + 1][1]);
          c.w[3] = pf_pack(st[2 * kk + 1][2], st[2 * kk + 1][3]);
          pa[kk] = c.f;
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            union { i16x4v s[2]; bf16x8v f; } vb;
#pragma unroll
            for (int u = 0; u < 2; ++u)
              vb.s[u] = pf_tr_read(vimg + kk * 32 * RB + v_base[u] +
                                   16 * ((2 * dt) ^ v_x[u]));
            o_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                pa[kk], vb.f, o_acc[dt], 0, 0, 0);
          }
      }
    }
    pf_barrier();
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  pf_barrier();

  // ---- row sums: the four lanes of a row, in g order ----
  float l_row = 0.f;
#pragma unroll
  for (int g = 0; g < 4; ++g) l_row += __shfl(l_run, li + 16 * g, WAVE);
  if (!live_s || !wave_live) {   // dead rows: no state, by select
    l_row = 0.f;
    m_run = -INFINITY;
  }

  if constexpr (KEYSPLIT) {
    // the four waves' states of the 16 rows, folded in wave order
    float* fimg = reinterpret_cast<float*>(smem);
    float* mine = fimg + wid * 16 * FLD;
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
    const int r = tid / CPR, ch = tid % CPR;
    if (tid < 16 * CPR && r < NR) {
      float M = -INFINITY;
#pragma unroll
      for (int w = 0; w < 4; ++w)
        M = fmaxf(M, fimg[(w * 16 + r) * FLD + D]);
      float L = 0.f, acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float* src = fimg + (w * 16 + r) * FLD;
        const float mw = src[D];
        const float e =
            (mw == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(mw - M);
        L = __builtin_fmaf(src[D + 1], e, L);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          acc[j] = __builtin_fmaf(src[ch * 8 + j], e, acc[j]);
      }
      const long gr = rows.global(r);
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
          ws[ws_ml0 + (gr * S + sp) * 2] =
              (M == -INFINITY) ? -INFINITY : M * PF_LN2;
          ws[ws_ml0 + (gr * S + sp) * 2 + 1] = L;
        }
      }
    }
  } else if (S == 1) {
    const float inv = (l_row > 0.f) ? 1.f / l_row : 0.f;
    bf16_t* oimg = reinterpret_cast<bf16_t*>(smem) + wid * 16 * OLD;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float ij = __shfl(inv, 4 * lg + j, WAVE);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const float val = (ij > 0.f) ? o_acc[dt][j] * ij : 0.f;
        oimg[(4 * lg + j) * OLD + dt * 16 + li] = f2bf(val);
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
            *reinterpret_cast<const uint4*>(oimg + r * OLD + ch * 8);
    }
  } else {
    // partial (m in natural-log units, l, unnormalised o)
    const float m_nat = (m_run == -INFINITY) ? -INFINITY : m_run * PF_LN2;
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

// ---- the quantizer of kv_fp8.hip (same arithmetic, same codes) ----
DEVINL uint2 pf_pack8(const float* x, float inv) {
  float y[8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    y[j] = fminf(fmaxf(x[j] * inv, -PF_MAX), PF_MAX);
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], hi, true);
  return make_uint2((uint32_t)lo, (uint32_t)hi);
}

DEVINL void pf_unpack_bf8(const bf16x8 v, float* f) {
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = bfbits2f(v.h[j]);
}

DEVINL float pf_amax8(const float* f) {
  float a = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) a = fmaxf(a, fabsf(f[j]));
  return a;
}

// max over the N consecutive lanes (N a power of two <= 16) that hold a row
template <int N>
DEVINL float pf_group_max(float a) {
#pragma unroll
  for (int off = N / 2; off > 0; off >>= 1)
    a = fmaxf(a, __shfl_xor(a, off, WAVE));
  return a;
}

// scale and 1/scale of a row from its amax (0, 0 for an all-zero row)
DEVINL void pf_row_scale(float amax, float* scale, float* inv) {
  const float s = amax / PF_MAX;
  *scale = (amax > 0.f) ? s : 0.f;
  *inv = (amax > 0.f) ? 1.f / s : 0.f;
}

constexpr int BLOCK_PF = 256;

// Pool row (page, head h, slot) of token position p of sequence b, or -1 for
// a dead token. The table is read only at an index inside it.
DEVINL long pf_dest(const int* page_table, int b, long p, bool live, int NP,
                    int P, int Hkv, int h) {
  if (!live || p < 0 || p >= (long)NP * PF_PAGE) return -1;
  const int pid = page_table[(long)b * NP + p / PF_PAGE];
  if (pid < 0 || pid >= P) return -1;
  return ((long)pid * Hkv + h) * PF_PAGE + p % PF_PAGE;
}

// Work item = 8 elements of one head row of k (which = 0) or v (which = 1).
template <int LPR>
PF_KERNEL void kv_quantize_append_paged_kernel(
    const bf16x8* __restrict__ k, const bf16x8* __restrict__ v,
    uint2* __restrict__ kpool, uint2* __restrict__ vpool,
    float* __restrict__ kscale, float* __restrict__ vscale,
    const int* __restrict__ pos, const int* __restrict__ qlens,
    const int* __restrict__ page_table, int B, int Tq, int NP, int P,
    int Hkv) {
  // nwork is a multiple of LPR and LPR divides the block: the lanes of a row
  // enter and leave the loop together
  const long nwork = (long)B * Tq * 2 * Hkv * LPR;
  for (long i = (long)blockIdx.x * BLOCK_PF + threadIdx.x; i < nwork;
       i += (long)gridDim.x * BLOCK_PF) {
    const long row = i / LPR;                   // (tok*2 + which)*Hkv + h
    const int c = (int)(i - row * LPR);
    const long tw = row / Hkv;                  // tok*2 + which
    const int h = (int)(row - tw * Hkv);
    const long tok = tw >> 1;                   // b*Tq + t
    const bool isv = tw & 1;
    const int b = (int)(tok / Tq);
    const int t = (int)(tok - (long)b * Tq);
    const long dst = pf_dest(page_table, b, (long)pos[b] + t, t < qlens[b],
                             NP, P, Hkv, h);
    float x[8];
    pf_unpack_bf8((isv ? v : k)[(tok * Hkv + h) * LPR + c], x);
    const float amax = pf_group_max<LPR>(pf_amax8(x));
    float scale, inv;
    pf_row_scale(amax, &scale, &inv);
    uint2 codes = pf_pack8(x, inv);
    if (!(amax > 0.f)) codes = make_uint2(0u, 0u);
    if (dst >= 0) {
      (isv ? vpool : kpool)[dst * LPR + c] = codes;
      if (c == 0) (isv ? vscale : kscale)[dst] = scale;
    }
  }
}

// Work item = one 8-wide vec of the first half of one head row of one token
// and its partner in the second half, as qkv_rope_append_fp8_kernel.
template <int HV /* (D/2)/8 */>
PF_KERNEL void qkv_rope_append_paged_fp8_kernel(
    const bf16x8* __restrict__ qkv, bf16x8* __restrict__ q,
    uint2* __restrict__ kpool, uint2* __restrict__ vpool,
    float* __restrict__ kscale, float* __restrict__ vscale,
    const float* __restrict__ tab_cos, const float* __restrict__ tab_sin,
    const int* __restrict__ pos, const int* __restrict__ qlens,
    const int* __restrict__ page_table, int B, int Tq, int NP, int P, int Hq,
    int Hkv) {
  constexpr int hv = HV;
  const int heads_total = Hq + 2 * Hkv;
  constexpr int dv8 = hv * 2;  // vecs per head (D/8)
  const long nwork = (long)B * Tq * heads_total * hv;
  for (long i = (long)blockIdx.x * BLOCK_PF + threadIdx.x; i < nwork;
       i += (long)gridDim.x * BLOCK_PF) {
    const long rowh = i / hv;                 // (b*Tq + t)*heads_total + h
    const int c = (int)(i - rowh * hv);
    const long tok = rowh / heads_total;      // b*Tq + t
    const int h = (int)(rowh - tok * heads_total);
    const int b = (int)(tok / Tq);
    const int t = (int)(tok - (long)b * Tq);
    const long p = (long)pos[b] + t;
    const bool isq = h < Hq;
    const bool isk = !isq && h < Hq + Hkv;
    const int hh = isq ? 0 : (isk ? h - Hq : h - Hq - Hkv);
    // liveness is a property of the token: uniform over the lanes of a row
    const long dst =
        pf_dest(page_table, b, p, t < qlens[b], NP, P, Hkv, hh);
    if (dst < 0) {
      if (isq) {  // zero q row, pools untouched
        bf16x8 z;
#pragma unroll
        for (int j = 0; j < 8; ++j) z.h[j] = 0;
        bf16x8* qd = q + (tok * Hq + h) * dv8;
        qd[c] = z;
        qd[c + hv] = z;
      }
      continue;
    }
    const bf16x8* src = qkv + rowh * dv8;
    bf16x8 o1 = src[c];
    bf16x8 o2 = src[c + hv];
    if (isq || isk) {
      const bf16x8 x1 = o1, x2 = o2;
      const float* cosr = tab_cos + p * (hv * 8);
      const float* sinr = tab_sin + p * (hv * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float cs = cosr[c * 8 + j];
        const float sn = sinr[c * 8 + j];
        const float a = bfbits2f(x1.h[j]);
        const float bb = bfbits2f(x2.h[j]);
        o1.h[j] = f2bfbits(a * cs - bb * sn);
        o2.h[j] = f2bfbits(bb * cs + a * sn);
      }
    }
    if (isq) {
      bf16x8* qd = q + (tok * Hq + h) * dv8;
      qd[c] = o1;
      qd[c + hv] = o2;
      continue;
    }
    // the bf16 row the bf16 kernels would have stored, quantized
    float f1[8], f2[8];
    pf_unpack_bf8(o1, f1);
    pf_unpack_bf8(o2, f2);
    const float amax = pf_group_max<HV>(fmaxf(pf_amax8(f1), pf_amax8(f2)));
    float scale, inv;
    pf_row_scale(amax, &scale, &inv);
    uint2 c1 = pf_pack8(f1, inv), c2 = pf_pack8(f2, inv);
    if (!(amax > 0.f)) c1 = c2 = make_uint2(0u, 0u);
    uint2* pool = isk ? kpool : vpool;
    pool[dst * dv8 + c] = c1;
    pool[dst * dv8 + c + hv] = c2;
    if (c == 0) (isk ? kscale : vscale)[dst] = scale;
  }
}

struct PfArgs {
  const void *q, *k, *v;
  const float *ks, *vs;
  const int *table, *lens, *qlens;
  void* out;
  float* ws;
  int B, Tq, NP, P, Hkv, num_splits, chunk;
  hipStream_t stream;
};

// The layout is picked here: up to 16 packed rows run key-split.
template <int D, int R>
void launch_paged_fp8(const PfArgs& a) {
  const float scale = 1.f / sqrtf((float)D);
  if (a.Tq * R <= 16) {
    dim3 grid(a.Hkv, a.B, a.num_splits);
    attn_paged_fp8_kernel<D, R, true><<<grid, PF_NTH, 0, a.stream>>>(
        (const bf16_t*)a.q, (const uint8_t*)a.k, (const uint8_t*)a.v, a.ks,
        a.vs, a.table, a.lens, a.qlens, (bf16_t*)a.out, a.ws, a.Tq, a.NP, a.P,
        a.Hkv, 1, a.chunk, scale);
  } else {
    const int MT = (a.Tq * R + 63) / 64;
    dim3 grid(a.Hkv * MT, a.B, a.num_splits);
    attn_paged_fp8_kernel<D, R, false><<<grid, PF_NTH, 0, a.stream>>>(
        (const bf16_t*)a.q, (const uint8_t*)a.k, (const uint8_t*)a.v, a.ks,
        a.vs, a.table, a.lens, a.qlens, (bf16_t*)a.out, a.ws, a.Tq, a.NP, a.P,
        a.Hkv, MT, a.chunk, scale);
  }
}

template <int D>
bool launch_paged_fp8_r(int R, const PfArgs& a) {
  switch (R) {
    case 1: launch_paged_fp8<D, 1>(a); return true;
    case 2: launch_paged_fp8<D, 2>(a); return true;
    case 4: launch_paged_fp8<D, 4>(a); return true;
    case 8: launch_paged_fp8<D, 8>(a); return true;
    default: return false;
  }
}

int pf_grid(long nwork) {
  long grid = (nwork + BLOCK_PF - 1) / BLOCK_PF;
  if (grid > 8192) grid = 8192;
  if (grid < 1) grid = 1;
  return (int)grid;
}

}  // namespace

extern "C" {

// ws: fp32, B*Tq*Hq*num_splits*(D+2) elements; unused when num_splits == 1.
hipError_t tok_attn_paged_fp8(const void* q, const void* kpool,
                              const void* vpool, const float* kscale,
                              const float* vscale, const int* page_table,
                              const int* lens, const int* qlens, void* out,
                              float* ws, int B, int Tq, int NP, int P, int Hq,
                              int Hkv, int D, int num_splits, int chunk,
                              hipStream_t stream) {
  if (Hkv < 1 || Hq % Hkv != 0 || Tq < 1 || B < 1 || NP < 1 || P < 1 ||
      num_splits < 1 || chunk < PF_PAGE || chunk % PF_PAGE != 0 ||
      (long)num_splits * chunk < (long)NP * PF_PAGE ||
      (long)NP * PF_PAGE >= (1L << 30))
    return hipErrorInvalidValue;
  const PfArgs a{q, kpool, vpool, kscale, vscale, page_table, lens, qlens,
                 out, ws, B, Tq, NP, P, Hkv, num_splits, chunk, stream};
  const int R = Hq / Hkv;
  bool ok = false;
  if (D == 128)
    ok = launch_paged_fp8_r<128>(R, a);
  else if (D == 64)
    ok = launch_paged_fp8_r<64>(R, a);
  if (!ok) return hipErrorInvalidValue;
  HIP_CHECK(hipGetLastError());
  if (num_splits > 1)
    HIP_CHECK(tok_attn_ragged_combine(ws, out, B * Tq, Hq, D, num_splits,
                                      stream));
  return hipSuccess;
}

hipError_t tok_kv_quantize_append_paged(const void* k, const void* v,
                                        void* kpool, void* vpool,
                                        float* kscale, float* vscale,
                                        const int* pos, const int* qlens,
                                        const int* page_table, int B, int Tq,
                                        int NP, int P, int Hkv, int D,
                                        hipStream_t stream) {
  const int grid = pf_grid((long)B * Tq * 2 * Hkv * (D / 8));
  if (D == 128)
    kv_quantize_append_paged_kernel<16><<<grid, BLOCK_PF, 0, stream>>>(
        (const bf16x8*)k, (const bf16x8*)v, (uint2*)kpool, (uint2*)vpool,
        kscale, vscale, pos, qlens, page_table, B, Tq, NP, P, Hkv);
  else if (D == 64)
    kv_quantize_append_paged_kernel<8><<<grid, BLOCK_PF, 0, stream>>>(
        (const bf16x8*)k, (const bf16x8*)v, (uint2*)kpool, (uint2*)vpool,
        kscale, vscale, pos, qlens, page_table, B, Tq, NP, P, Hkv);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t tok_qkv_rope_append_paged_fp8(
    const void* qkv, void* q, void* kpool, void* vpool, float* kscale,
    float* vscale, const float* cos_tab, const float* sin_tab, const int* pos,
    const int* qlens, const int* page_table, int B, int Tq, int NP, int P,
    int Hq, int Hkv, int D, hipStream_t stream) {
  const int grid = pf_grid((long)B * Tq * (Hq + 2 * Hkv) * ((D / 2) / 8));
  if (D == 128)
    qkv_rope_append_paged_fp8_kernel<8><<<grid, BLOCK_PF, 0, stream>>>(
        (const bf16x8*)qkv, (bf16x8*)q, (uint2*)kpool, (uint2*)vpool, kscale,
        vscale, cos_tab, sin_tab, pos, qlens, page_table, B, Tq, NP, P, Hq,
        Hkv);
  else if (D == 64)
    qkv_rope_append_paged_fp8_kernel<4><<<grid, BLOCK_PF, 0, stream>>>(
        (const bf16x8*)qkv, (bf16x8*)q, (uint2*)kpool, (uint2*)vpool, kscale,
        vscale, cos_tab, sin_tab, pos, qlens, page_table, B, Tq, NP, P, Hq,
        Hkv);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}
}
