// FP8 (OCP e4m3) paged KV cache on MI355X (gfx950): MFMA attention over e4m3
// pages for decode (Tq = 1) and chunked prefill (Tq > 1). The two appends that
// write tokens into their pages are in kv_fp8.hip, next to the quantizer.
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
//   attn_paged_fp8_kernel<128,1,false>          182     0    69  69632  2
//   attn_paged_fp8_kernel<128,2|4|8,false>      182     0    74  69632  2
//   attn_paged_fp8_kernel<64,1,true>             68     0    65  28672  5
//   attn_paged_fp8_kernel<64,2|4|8,true>         68     0    68  28672  5
//   attn_paged_fp8_kernel<64,1,false>           130     0    68  36864  3
//   attn_paged_fp8_kernel<64,2|4|8,false>       130     0    73  36864  3
// (waves/SIMD as the compiler reports it; LDS bounds it in the key-split
// layout, three blocks per CU at D = 128 where the bf16 kernel has two; the
// row layout keeps two, with the codes of 16 K and 16 V rows in registers on
// their way to the image.) In the .s every tile loop holds exactly one
// s_waitcnt vmcnt(6) (vmcnt(4) at D = 64) in front of its first barrier and no
// vmcnt(0). The widening that shipped is v_cvt_scalef32_pk_bf16_fp8: exact on
// the hardware for every non-NaN code (tests/test_attention_paged_fp8_gpu.py,
// random codes over all byte values against fp64).
#include "attn_kv_tile.h"

extern "C" hipError_t tok_attn_ragged_combine(const float* ws, void* out,
                                              int rows, int Hq, int D,
                                              int num_splits,
                                              hipStream_t stream);

namespace {

// chunk swizzle of the codes image, r in [0, 16)
template <int D>
DEVINL int pf_cswz(int r) {
  return D == 128 ? (r >> 1) & 7 : (r >> 2) & 3;
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
    const int x = kt_swz<D>(row);
    *reinterpret_cast<uint4*>(dst + 16 * ((2 * cc) ^ x)) = lo;
    *reinterpret_cast<uint4*>(dst + 16 * ((2 * cc + 1) ^ x)) = hi;
  }
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
  constexpr int CT = KT_PAGE * D, NJ = CT / 4096, RPS = 4096 / D;
  const long slab = (long)min(max(raw_id, 0), P - 1) * Hkv + hkv;
  const char* kb = kt_uniform(pools.k + slab * CT);
  const char* vb = kt_uniform(pools.v + slab * CT);
  const char* ksb = kt_uniform(pools.ks + slab * (KT_PAGE * 4));
  const char* vsb = kt_uniform(pools.vs + slab * (KT_PAGE * 4));
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int slot = min(j * RPS + d_row, last_slot);
    const uint32_t voff = (uint32_t)slot * D + d_ch * 16;
    kt_glds16(voff, kb, dst + j * 4096);
    kt_glds16(voff, vb, dst + CT + j * 4096);
  }
  const uint32_t soff = (uint32_t)min(lane, last_slot) * 4;
  kt_glds4(soff, ksb, sdst);
  kt_glds4(soff, vsb, sdst + KT_PAGE * 4);
}

// The segments of attn_kv_tile.h around this format's staging, LDS plan,
// widening, K fragments from codes and row scales.
template <int D, int R, bool KEYSPLIT>
KT_KERNEL __launch_bounds__(KT_NTH, 2) void attn_paged_fp8_kernel(
    const bf16_t* __restrict__ q, const uint8_t* __restrict__ kpool,
    const uint8_t* __restrict__ vpool, const float* __restrict__ kscale,
    const float* __restrict__ vscale, const int* __restrict__ page_table,
    const int* __restrict__ lens, const int* __restrict__ qlens,
    bf16_t* __restrict__ out, float* __restrict__ ws, int Tq, int NP, int P,
    int Hkv, int MT, int chunk, float scale) {
  constexpr int RB = D * 2;                    // bytes per bf16 image row
  constexpr int CT = KT_PAGE * D;              // one K or V code slab
  constexpr int NJ = CT / 4096;                // 16-byte DMAs per slab
  constexpr int CPC = D / 16;                  // 16-byte chunks per codes row
  constexpr int SCB = 4 * 2 * KT_PAGE * 4;     // four waves' scale strip pairs
  constexpr int STAGE = 2 * CT + SCB;          // one staging buffer
  constexpr int IMG = (KEYSPLIT ? 1 : 2) * KT_PAGE * RB;  // bf16 image
  constexpr int KS = D / 32;                   // k steps of S^T
  constexpr int DT = D / 16;                   // d tiles of O
  constexpr int NKT = KEYSPLIT ? 1 : 4;        // 16-key groups per wave
  constexpr int SMEM = 2 * STAGE + IMG;
  __shared__ __attribute__((aligned(1024))) char smem[SMEM];
  static_assert(2 * STAGE <= 65536, "DMA targets within 16 address bits");
  static_assert(4 * 16 * (D + 8) * 2 <= SMEM, "epilogue image fits");
  static_assert(4 * 16 * (D + 2) * 4 <= SMEM, "fold image fits");

  const KtBlock<D, R, KEYSPLIT> g(lens, qlens, Tq, NP * KT_PAGE, Hkv, MT,
                                  chunk);
  if (g.dead()) {
    kt_write_dead(g, out, ws);
    return;
  }
  const KtWave w(g);
  const int lane = g.lane, wid = g.wid, li = g.li, lg = g.lg;

  bf16x8v qf[KS];
  kt_load_q(qf, q, g, w);

  // ---- DMA geometry ----
  const uint32_t lds_base = __builtin_amdgcn_readfirstlane(
      (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem);
  const uint32_t lds0 = lds_base + wid * 1024;              // codes share
  const uint32_t sds0 = lds_base + 2 * CT + wid * (SCB / 4);  // scale strips
  const int d_row = g.tid / CPC;                       // slot within a 4 KiB
  const int d_ch = (g.tid % CPC) ^ pf_cswz<D>(d_row & 15);
  const PfPools pools{reinterpret_cast<const char*>(kpool),
                      reinterpret_cast<const char*>(vpool),
                      reinterpret_cast<const char*>(kscale),
                      reinterpret_cast<const char*>(vscale)};
  const int* tab = page_table + (long)g.b * NP;
  const int pg0 = g.kbeg / KT_PAGE;                    // < NP: kbeg < kend <= n
  const int ntiles = g.ntiles();
  const int krem = g.kend - 1 - g.kbeg;                // last row, from kbeg

  // key-split K: 8 codes of row 16w + li, bytes within a codes slab
  uint32_t kc_off[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
    kc_off[ks] = (16 * wid + li) * D +
                 16 * ((2 * ks + (lg >> 1)) ^ pf_cswz<D>(li)) + 8 * (lg & 1);
  const KtFrag<D, KEYSPLIT> fr(lane, wid);             // reads of the image
  char* const img = smem + 2 * STAGE;                  // bf16 image: K, then V
  char* const vimg = img + (KEYSPLIT ? 0 : KT_PAGE * RB);

  const float c2 = scale * KT_LOG2E;
  const KtLog2M mu;                                    // scores carry c2
  float m_run = -INFINITY, l_run = 0.f;
  f32x4 o_acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o_acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  pf_stage<D>(pools, tab[pg0], P, Hkv, g.hkv, lds0, sds0,
              min(KT_PAGE - 1, krem), d_row, d_ch, lane);
  int id_next = tab[pg0 + min(1, ntiles - 1)];         // raw id of tile t + 1
  kt_pin_q(qf);
  for (int t = 0; t < ntiles; ++t) {
    const int buf = t & 1;
    pf_stage<D>(pools, id_next, P, Hkv, g.hkv, lds0 + (buf ^ 1) * STAGE,
                sds0 + (buf ^ 1) * STAGE,
                min(KT_PAGE - 1, krem - min(t + 1, ntiles - 1) * KT_PAGE),
                d_row, d_ch, lane);
    id_next = tab[pg0 + min(t + 2, ntiles - 1)];
    if (NJ == 2)
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    kt_barrier();

    const char* cbuf = smem + buf * STAGE;             // K codes, V codes
    const char* sbuf = cbuf + 2 * CT + wid * (SCB / 4);  // own kscale, vscale
    if constexpr (!KEYSPLIT) {
      pf_widen16<D>(cbuf + wid * 16 * D, img + wid * 16 * RB, lane);
      pf_widen16<D>(cbuf + CT + wid * 16 * D, vimg + wid * 16 * RB, lane);
      kt_barrier();
    }

    const int kw0 = g.kbeg + t * KT_PAGE + 16 * w.kt0;  // wave's first key
    if (w.wave_live && kw0 <= w.lim_last) {
      if constexpr (KEYSPLIT)  // own 16 V rows -> own strip, read back below
        pf_widen16<D>(cbuf + CT + wid * 16 * D, vimg + wid * 16 * RB, lane);

      // S^T = K Q^T over the codes
      f32x4 st[NKT];
      if constexpr (KEYSPLIT) {
        st[0] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const uint2 raw = *reinterpret_cast<const uint2*>(cbuf + kc_off[ks]);
          union { uint32_t w[4]; bf16x8v f; } c;
          c.w[0] = pf_widen2<false>(raw.x);
          c.w[1] = pf_widen2<true>(raw.x);
          c.w[2] = pf_widen2<false>(raw.y);
          c.w[3] = pf_widen2<true>(raw.y);
          st[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(c.f, qf[ks], st[0],
                                                          0, 0, 0);
        }
      } else {
        kt_scores<D>(st, img, fr.k_off, qf);
      }

      // the row scales of the lane's keys 16(kt0 + kt) + 4g .. + 3
      f32x4 vsc[NKT];
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        const char* sp4 = sbuf + (16 * (w.kt0 + kt) + 4 * lg) * 4;
        const f32x4 ksc = *reinterpret_cast<const f32x4*>(sp4);
        vsc[kt] = *reinterpret_cast<const f32x4*>(sp4 + KT_PAGE * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) st[kt][j] *= ksc[j] * c2;
      }

      const float alpha = kt_softmax_step(st, m_run, l_run, mu, kw0, lg, w);
      // vscale once, before P's rounding; l has summed the unscaled p
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) st[kt][j] *= vsc[kt][j];
      kt_rescale(o_acc, alpha, lg);

      if constexpr (KEYSPLIT) {
        // the strip this wave wrote above is in LDS before it is read
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        kt_pv16<D>(o_acc, st[0], vimg, fr.v_base[0], fr.v_x[0]);
      } else {
        kt_pv64<D>(o_acc, st, vimg, fr.v_base, fr.v_x);
      }
    }
    kt_barrier();
  }
  kt_finish(smem, o_acc, m_run, l_run, g, w, mu, out, ws);
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
    attn_paged_fp8_kernel<D, R, true><<<grid, KT_NTH, 0, a.stream>>>(
        (const bf16_t*)a.q, (const uint8_t*)a.k, (const uint8_t*)a.v, a.ks,
        a.vs, a.table, a.lens, a.qlens, (bf16_t*)a.out, a.ws, a.Tq, a.NP, a.P,
        a.Hkv, 1, a.chunk, scale);
  } else {
    const int MT = (a.Tq * R + 63) / 64;
    dim3 grid(a.Hkv * MT, a.B, a.num_splits);
    attn_paged_fp8_kernel<D, R, false><<<grid, KT_NTH, 0, a.stream>>>(
        (const bf16_t*)a.q, (const uint8_t*)a.k, (const uint8_t*)a.v, a.ks,
        a.vs, a.table, a.lens, a.qlens, (bf16_t*)a.out, a.ws, a.Tq, a.NP, a.P,
        a.Hkv, MT, a.chunk, scale);
  }
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
      num_splits < 1 || chunk < KT_PAGE || chunk % KT_PAGE != 0 ||
      (long)num_splits * chunk < (long)NP * KT_PAGE ||
      (long)NP * KT_PAGE >= (1L << 30))
    return hipErrorInvalidValue;
  const PfArgs a{q, kpool, vpool, kscale, vscale, page_table, lens, qlens,
                 out, ws, B, Tq, NP, P, Hkv, num_splits, chunk, stream};
  const bool ok = kt_dispatch(D, Hq / Hkv, [&](auto d, auto r) {
    launch_paged_fp8<decltype(d)::value, decltype(r)::value>(a);
  });
  if (!ok) return hipErrorInvalidValue;
  HIP_CHECK(hipGetLastError());
  if (num_splits > 1)
    HIP_CHECK(tok_attn_ragged_combine(ws, out, B * Tq, Hq, D, num_splits,
                                      stream));
  return hipSuccess;
}
}
