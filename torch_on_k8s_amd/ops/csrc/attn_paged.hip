// Paged KV cache for ragged generation on MI355X (gfx950): attention over
// 64-token pages, in a row layout (chunked prefill) and a key-split layout
// (decode), and the append that writes new tokens into their pages.
//
//   attn_paged_kernel<D, R, KEYSPLIT>   grid (Hkv * row_tiles, B, splits), 256 thr
//     q [B,Tq,Hq,D]; kpool/vpool [P,Hkv,64,D] bf16: one (page, kv head) is a
//     contiguous 64*D*2-byte slab; page_table [B,NP] int32, lens/qlens [B]
//     int32, all on the device and never read by the host. Logical row t of
//     sequence b lives in page page_table[b, t / 64], slot t % 64.
//     Tmax = 64 NP. A page id is clamped into [0, P): a wrong table gives
//     wrong numbers, never a fault.
//     The design written up in attn_kv_tile.h (work split, both layouts,
//     operand layouts, LDS image, bank argument, softmax, fold, epilogue);
//     the launcher picks the key-split layout for Tq * R <= 16. The body is
//     NOT yet an instance of kt_attn: as one it computed the same bits but
//     ran 3-5 % slower than this text on the bandwidth-bound row-layout
//     lines (Tq = 8, equal lengths, T = 32768; profiles/README.md), so it
//     stays as it was, on the shared primitives, until that is understood.
//
// Staging. A key tile IS a page. The id of tile t + 2 is read from the table
// one iteration ahead (a uniform scalar load whose wait falls on the next
// iteration's first LDS wait), clamped, and turned into the two slab bases.
// The source slot is min(slot, last valid slot of the tile): 63 everywhere
// but in the tile that holds row kend - 1, so a row >= n of a tail page (NaN
// from an earlier owner) never enters LDS. A slab is contiguous, so the DMA
// offset is slot * D*2 + chunk * 16 and needs no row stride.
//
//   qkv_rope_append_paged_kernel   grid-stride, 256 threads
//     qkv_rope_append_chunk_kernel with the destination looked up in the
//     table (the rule of KtPagedDest, attn_kv_tile.h; see attn_extend.hip
//     for why the body is not shared); per element the same arithmetic.
//     Token i of sequence b is live iff i < qlens[b],
//     0 <= pos[b] + i < 64 NP and its table entry is in [0, P);
//     a dead token writes nothing (a clamped write would land in someone
//     else's page) and gets a zero q row.
//
// Resources (hipcc -O3 --offload-arch=gfx950,
// -Rpass-analysis=kernel-resource-usage; scratch is 0 B everywhere):
//   kernel                                  VGPR  AGPR  SGPR  LDS B  waves/SIMD
//   attn_paged_kernel<128,1|2|4|8,true>      100     0    59  65536  2
//   attn_paged_kernel<128,1,false>           139     0    61  65536  2
//   attn_paged_kernel<128,2|4|8,false>       139     0    63  65536  2
//   attn_paged_kernel<64,1|4|8,true>          67     0    59  32768  5
//   attn_paged_kernel<64,2,true>              69     0    59  32768  5
//   attn_paged_kernel<64,1,false>             93     0    61  32768  5
//   attn_paged_kernel<64,2|4|8,false>         93     0    63  32768  5
//   qkv_rope_append_paged_kernel              51     0    72      0  8
// (waves/SIMD as the compiler reports it: LDS bounds it, two blocks per CU at
// D = 128 and five at D = 64.) In the .s every tile loop holds exactly one
// s_waitcnt vmcnt(8) (vmcnt(4) at D = 64) in front of its first barrier and no
// vmcnt(0); the table reads are s_load_dword. The compiler's own wait for the
// q loads would be a vmcnt(0) inside the loop (it does not count the
// inline-asm DMAs), so q is "used" by an empty asm before the loop.
#include "attn_kv_tile.h"

extern "C" hipError_t tok_attn_ragged_combine(const float* ws, void* out,
                                              int rows, int Hq, int D,
                                              int num_splits,
                                              hipStream_t stream);

namespace {

// The K and the V slab of page raw_id (clamped into [0, P): never a fault)
// of the kv head at head_off, slots clamped to last_slot, into the pair of
// tiles at LDS address dst (wave part included).
template <int D>
DEVINL void pg_stage(const char* kpool, const char* vpool, int raw_id, int P,
                     long page_bytes, long head_off, uint32_t dst,
                     int last_slot, int d_row, int d_ch) {
  constexpr int TILE = KT_PAGE * D * 2, NJ = TILE / 4096, RPS = 4096 / (D * 2);
  const long slab = min(max(raw_id, 0), P - 1) * page_bytes + head_off;
  const char* kb = kt_uniform(kpool + slab);
  const char* vb = kt_uniform(vpool + slab);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int slot = min(j * RPS + d_row, last_slot);
    const uint32_t voff = (uint32_t)slot * (D * 2) + d_ch * 16;
    kt_glds16(voff, kb, dst + j * 4096);
    kt_glds16(voff, vb, dst + TILE + j * 4096);
  }
}

template <int D, int R, bool KEYSPLIT>
KT_KERNEL __launch_bounds__(KT_NTH, 2) void attn_paged_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ kpool,
    const bf16_t* __restrict__ vpool, const int* __restrict__ page_table,
    const int* __restrict__ lens, const int* __restrict__ qlens,
    bf16_t* __restrict__ out, float* __restrict__ ws, int Tq, int NP, int P,
    int Hkv, int MT, int chunk, float scale) {
  constexpr int RB = D * 2;                    // bytes per tile row
  constexpr int TILE = KT_PAGE * RB;           // one K or V slab
  constexpr int NJ = TILE / 4096;              // DMA instructions per slab
  constexpr int CPR = D / 8;                   // 16-byte chunks per row
  constexpr int KS = D / 32;                   // k steps of S^T
  constexpr int DT = D / 16;                   // d tiles of O
  constexpr int OLD = D + 8;                   // bf16 epilogue row, elements
  constexpr int FLD = D + 2;                   // fp32 fold row: o[D], m, l
  constexpr int BM = KEYSPLIT ? 16 : 64;       // packed q rows per block
  constexpr int NKT = KEYSPLIT ? 1 : 4;        // 16-key groups per wave
  __shared__ __attribute__((aligned(1024))) char smem[4 * TILE];
  static_assert(4 * 16 * OLD * 2 <= 4 * TILE, "epilogue image fits");
  static_assert(4 * 16 * FLD * 4 <= 4 * TILE, "fold image fits");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int hkv = blockIdx.x / MT, mt = blockIdx.x - hkv * MT;
  const int b = blockIdx.y, sp = blockIdx.z;
  const int S = gridDim.z;
  const int Hq = Hkv * R;
  const int NR = Tq * R;                       // packed rows of this kv head
  const int Tmax = NP * KT_PAGE;

  const int n = min(max(lens[b], 0), Tmax);
  const int m = min(max(qlens[b], 0), min(Tq, n));
  const int base_pos = n - m;                  // position of query 0

  const int row_blk = mt * BM;
  const int i_first = row_blk / R;
  const int i_last = min(m - 1, (row_blk + BM - 1) / R);
  const int p_last = base_pos + i_last;
  const int kbeg = sp * chunk;
  const int kend = min(kbeg + chunk, p_last + 1);

  const KtRows<R> rows{(long)b * Tq, Hq, hkv * R};
  const long ws_ml0 = (long)gridDim.y * Tq * Hq * S * D;

  if (i_first >= m || kbeg >= kend) {  // block-uniform: nothing to attend to
    for (int idx = tid; idx < BM * CPR; idx += KT_NTH) {
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
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane(
      (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem +
      wid * 1024);
  const int d_row = tid / CPR;                         // slot within a 4 KiB
  const int d_ch = (tid % CPR) ^ kt_swz<D>(d_row & 15);
  const char* kbytes = reinterpret_cast<const char*>(kpool);
  const char* vbytes = reinterpret_cast<const char*>(vpool);
  const int* tab = page_table + (long)b * NP;
  const int pg0 = kbeg / KT_PAGE;                      // < NP: kbeg < kend <= n
  const int ntiles = (kend - kbeg + KT_PAGE - 1) / KT_PAGE;
  const long head_off = (long)hkv * TILE;
  const int krem = kend - 1 - kbeg;                    // last row, from kbeg

  // ---- fragment read offsets (bytes within a tile) ----
  uint32_t k_off[KS];   // + kt * 16 * RB
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
    k_off[ks] = li * RB + 16 * ((4 * ks + lg) ^ kt_swz<D>(li));
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
      v_x[u] = (tp >> 1) ^ kt_swz<D>(r & 15);
    }
  }

  const float c2 = scale * KT_LOG2E;
  float m_run = -INFINITY, l_run = 0.f;
  f32x4 o_acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o_acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const long page_bytes = (long)Hkv * TILE;
  pg_stage<D>(kbytes, vbytes, tab[pg0], P, page_bytes, head_off, lds0,
              min(KT_PAGE - 1, krem), d_row, d_ch);
  int id_next = tab[pg0 + min(1, ntiles - 1)];         // raw id of tile t + 1
  // Use q here, so that the compiler's wait for the q loads sits before the
  // loop (tile 0 must land anyway) and not as a vmcnt(0) inside it.
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks]));
  for (int t = 0; t < ntiles; ++t) {
    const int buf = t & 1;
    pg_stage<D>(kbytes, vbytes, id_next, P, page_bytes, head_off,
                lds0 + (buf ^ 1) * 2 * TILE,
                min(KT_PAGE - 1, krem - min(t + 1, ntiles - 1) * KT_PAGE),
                d_row, d_ch);
    id_next = tab[pg0 + min(t + 2, ntiles - 1)];
    if (NJ == 4)
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    kt_barrier();

    const int k0 = kbeg + t * KT_PAGE;
    const int kw0 = k0 + 16 * kt0;                     // wave's first key
    if (wave_live && kw0 <= lim_last) {
      const char* kt_lds = smem + buf * 2 * TILE + kt0 * 16 * RB;
      const char* vt_lds = smem + buf * 2 * TILE + TILE;

      // S^T = K Q^T: st[kt][j] = score of (key kw0 + 16kt + 4g + j, row li)
      f32x4 st[NKT];
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
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
      const float neg_mc = (m_new == -INFINITY) ? 0.f : -m_new * c2;
      const float alpha =
          __builtin_amdgcn_exp2f(__builtin_fmaf(m_run, c2, neg_mc));
      m_run = m_new;

      float psum = 0.f;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float p = __builtin_amdgcn_exp2f(
              __builtin_fmaf(st[kt][j], c2, neg_mc));
          if (needs_mask)
            p = (kw0 + 16 * kt + 4 * lg + j <= lim_s) ? p : 0.f;
          st[kt][j] = p;
          psum += p;
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
        // P of the wave's 16 keys IS the A operand of the K = 16 MFMA
        union { uint32_t w[2]; i16x4v f; } pa;
        pa.w[0] = kt_pack(st[0][0], st[0][1]);
        pa.w[1] = kt_pack(st[0][2], st[0][3]);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const i16x4v vb =
              kt_tr_read(vt_lds + v_base[0] + 16 * ((2 * dt) ^ v_x[0]));
          o_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(
              pa.f, vb, o_acc[dt], 0, 0, 0);
        }
      } else {
        // P as the A operand: one rounding to bf16
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
          for (int dt = 0; dt < DT; ++dt) {
            union { i16x4v s[2]; bf16x8v f; } vb;
#pragma unroll
            for (int u = 0; u < 2; ++u)
              vb.s[u] = kt_tr_read(vt_lds + kk * 32 * RB + v_base[u] +
                                   16 * ((2 * dt) ^ v_x[u]));
            o_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                pa[kk], vb.f, o_acc[dt], 0, 0, 0);
          }
      }
    }
    kt_barrier();
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  kt_barrier();

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
    float* img = reinterpret_cast<float*>(smem);
    float* mine = img + wid * 16 * FLD;
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
        M = fmaxf(M, img[(w * 16 + r) * FLD + D]);
      float L = 0.f, acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float* src = img + (w * 16 + r) * FLD;
        const float mw = src[D];
        const float e = (mw == -INFINITY)
                            ? 0.f
                            : __builtin_amdgcn_exp2f((mw - M) * c2);
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
              (M == -INFINITY) ? -INFINITY : M * scale;
          ws[ws_ml0 + (gr * S + sp) * 2 + 1] = L;
        }
      }
    }
  } else if (S == 1) {
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

// Work item = one 8-wide vec of the first half of one head row of one token
// and its partner in the second half, as qkv_rope_append_chunk_kernel.
KT_KERNEL void qkv_rope_append_paged_kernel(
    const bf16x8* __restrict__ qkv, bf16x8* __restrict__ q,
    bf16x8* __restrict__ kpool, bf16x8* __restrict__ vpool,
    const float* __restrict__ tab_cos, const float* __restrict__ tab_sin,
    const int* __restrict__ pos, const int* __restrict__ qlens,
    const int* __restrict__ page_table, int B, int Tq, int NP, int P, int Hq,
    int Hkv, int hv /* (D/2)/8 */) {
  const int heads_total = Hq + 2 * Hkv;
  const int dv8 = hv * 2;  // vecs per head (D/8)
  const long nwork = (long)B * Tq * heads_total * hv;
  for (long i = (long)blockIdx.x * KT_NTH + threadIdx.x; i < nwork;
       i += (long)gridDim.x * KT_NTH) {
    const long rowh = i / hv;                 // (b*Tq + t)*heads_total + h
    const int c = (int)(i - rowh * hv);
    const long tok = rowh / heads_total;      // b*Tq + t
    const int h = (int)(rowh - tok * heads_total);
    const int b = (int)(tok / Tq);
    const int t = (int)(tok - (long)b * Tq);
    const long p = (long)pos[b] + t;
    bool live = t < qlens[b] && p >= 0 && p < (long)NP * KT_PAGE;
    int pid = -1;
    if (live) {  // the table is read only at an index inside it
      pid = page_table[(long)b * NP + p / KT_PAGE];
      live = pid >= 0 && pid < P;
    }
    bf16x8* dst;
    bool rot;
    if (h < Hq) {
      dst = q + (tok * Hq + h) * dv8;
      rot = true;
      if (!live) {  // zero q row, pools untouched
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
      dst = (isk ? kpool : vpool) +
            (((long)pid * Hkv + hh) * KT_PAGE + (p % KT_PAGE)) * dv8;
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

}  // namespace

extern "C" {

// ws: fp32, B*Tq*Hq*num_splits*(D+2) elements; unused when num_splits == 1.
hipError_t tok_attn_paged(const void* q, const void* kpool, const void* vpool,
                          const int* page_table, const int* lens,
                          const int* qlens, void* out, float* ws, int B,
                          int Tq, int NP, int P, int Hq, int Hkv, int D,
                          int num_splits, int chunk, hipStream_t stream) {
  if (Hkv < 1 || Hq % Hkv != 0 || Tq < 1 || B < 1 || NP < 1 || P < 1 ||
      num_splits < 1 || chunk < KT_PAGE || chunk % KT_PAGE != 0 ||
      (long)num_splits * chunk < (long)NP * KT_PAGE ||
      (long)NP * KT_PAGE >= (1L << 30))
    return hipErrorInvalidValue;
  const bool ok = kt_dispatch(D, Hq / Hkv, [&](auto d, auto r) {
    constexpr int DD = decltype(d)::value, R = decltype(r)::value;
    const float scale = 1.f / sqrtf((float)DD);
    // The layout is picked here: up to 16 packed rows run key-split.
    if (Tq * R <= 16) {
      dim3 grid(Hkv, B, num_splits);
      attn_paged_kernel<DD, R, true><<<grid, KT_NTH, 0, stream>>>(
          (const bf16_t*)q, (const bf16_t*)kpool, (const bf16_t*)vpool,
          page_table, lens, qlens, (bf16_t*)out, ws, Tq, NP, P, Hkv, 1, chunk,
          scale);
    } else {
      const int MT = (Tq * R + 63) / 64;
      dim3 grid(Hkv * MT, B, num_splits);
      attn_paged_kernel<DD, R, false><<<grid, KT_NTH, 0, stream>>>(
          (const bf16_t*)q, (const bf16_t*)kpool, (const bf16_t*)vpool,
          page_table, lens, qlens, (bf16_t*)out, ws, Tq, NP, P, Hkv, MT, chunk,
          scale);
    }
  });
  if (!ok) return hipErrorInvalidValue;
  HIP_CHECK(hipGetLastError());
  if (num_splits > 1)
    HIP_CHECK(tok_attn_ragged_combine(ws, out, B * Tq, Hq, D, num_splits,
                                      stream));
  return hipSuccess;
}

hipError_t tok_qkv_rope_append_paged(const void* qkv, void* q, void* kpool,
                                     void* vpool, const float* cos_tab,
                                     const float* sin_tab, const int* pos,
                                     const int* qlens, const int* page_table,
                                     int B, int Tq, int NP, int P, int Hq,
                                     int Hkv, int D, hipStream_t stream) {
  const int hv = (D / 2) / 8;
  const int grid = kt_append_grid((long)B * Tq * (Hq + 2 * Hkv) * hv);
  qkv_rope_append_paged_kernel<<<grid, KT_NTH, 0, stream>>>(
      (const bf16x8*)qkv, (bf16x8*)q, (bf16x8*)kpool, (bf16x8*)vpool, cos_tab,
      sin_tab, pos, qlens, page_table, B, Tq, NP, P, Hq, Hkv, hv);
  return hipGetLastError();
}
}
