// Flash attention (causal, GQA/MHA) for MI355X (gfx950) - fwd + bwd.
//
// Architecture (v3/v4; progression + measurements in profiles/README.md;
// the default forward is attn_fwd_kernel_v4, which keeps this structure):
//  * mfma_f32_32x32x16_bf16 tiles with SWAPPED operands: S^T = K*Q^T so
//    each lane owns ONE q row; online softmax is fully in-register (an
//    in-lane chain + one half-wave shuffle; no cross-lane reduce, no P
//    round trip through LDS). Fragment layouts verified on hardware by
//    mfma_probe.hip.
//  * P / dS^T are repacked from the MFMA C-layout to the next MFMA's
//    A-layout with v_cvt_pk_bf16_f32 pairs + permlane32_swap (guide T12):
//    C-layout element r of half h sits at k=(r&3)+8*(r>>2)+4h; one swap
//    fixes two A-fragment words.
//  * Q (fwd), K/V (dq) and K (dv/dk) live in registers as the MFMA
//    B-operand; tiles consumed d-major (V fwd, K^T/Q^T/dO^T bwd) are
//    read from PRE-TRANSPOSED [B,H,D,S_pad] planes (transpose.hip) so
//    all LDS staging is vectorized b128 writes - the in-kernel scalar
//    transpose scatter measured ~20 LDS bank-conflict cycles per MFMA.
//  * LDS tiles are double-buffered (one barrier per tile; the next
//    tile's write overlaps other waves' compute) and XOR-swizzled on the
//    FULL tile offset ((row&15)<<4: conflict-free 16-lane b128 groups;
//    bit 7 swaps row parity in-tile for 128-B rows).
//  * async-stage prefetch (T14), s_setprio around MFMA clusters (T5),
//    defer-max online softmax (T13), interior tiles skip masking.
//  * Backward: flash recompute scheme in a Dsum = rowsum(dO*O) preprocess,
//    one fused dK+dV kernel (64 keys per wave, 1 wave/SIMD, dK^T and dV^T
//    in 256 accumulator registers, row constants as the accumulators'
//    start values) and a deterministic dQ kernel over q tiles. The older
//    split dV / dK pair (2 waves/SIMD, S recomputed in each) stays behind
//    tok_attn_bwd's `split` selector for A/B timing, and a 4-wave dQ
//    kernel (64 q rows per wave, measured slower) behind `dq_variant`.
//    All kernels: 0 scratch spill.
//  * fwd v4, fused dK+dV and dQ take their block from xcd_block_index():
//    the blocks that share a kv head's tiles run on one XCD's L2.
//  * Packed documents (template flag DOC on fwd v4, fused dK+dV and the
//    8-wave dQ): optional int32 [B,S] doc_start / doc_end bounds add a
//    second cut next to the causal one - query i sees keys doc_start[i]..i.
//    Key tiles of earlier documents are never staged. See DocRows and the
//    fused kernel; measurements in profiles/attn_docs.log.
//
// Measured (B=2 S=4096 Hq=32 Hkv=8 D=128 causal, random data): fwd v3
// 358-371 TF (parity with torch's aotriton flash), v4 see
// profiles/attn_fwd_v4.log; bwd incl. the three
// operand transposes 292-294 TF fused, 212-214 TF with the split pair
// (profiles/attn_dkdv.log).
#include "common.h"

namespace {

using bf16x8v = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int BN = 64;    // kv rows per LDS tile (fwd/dq); q rows in dkdv
constexpr int NW = 8;     // waves per block
constexpr int NTHREADS = NW * WAVE;   // 512
constexpr int BM = NW * 16;           // 128 rows owned per block (1 strip/wave)
constexpr float NEG_INF = -INFINITY;

// Swizzled tile offset: (row*RB + col) ^ ((row&15)<<4) spreads a 16-lane
// ds_read_b128 group over 16 16-B slots (conflict-free when the group's
// rows are distinct mod 16, guide §6 G4). The XOR is applied to the FULL
// tile offset: for 128-B rows bit 7 of the mask swaps row parity, which
// keeps the mapping a bijection INSIDE the tile (XOR-ing only the
// byte-in-row would escape the last rows' allocation).
DEVINL int swz_off(int row, int row_bytes, int byte_in_row) {
  return (row * row_bytes + byte_in_row) ^ ((row & 15) << 4);
}

DEVINL bf16x8v as_frag(uint4 raw) {
  union { uint4 u; bf16x8v f; } c;
  c.u = raw;
  return c.f;
}

// XCD-aware block order. Workgroups go to the 8 XCDs round-robin by linear
// id, so the blocks that share one kv head's tiles (the q blocks and q
// heads of a kv head in fwd / dQ, the key blocks of a kv head in dK+dV)
// land on eight different L2s, and each of them fetches those tiles again.
// Remapped, XCD r works through the r-th contiguous eighth of the grid: the
// blocks in flight on one XCD share one or two kv heads. Measured on the
// dQ kernel at B=8 S=4096: whole backward 8.91 -> 7.70 ms
// (profiles/attn_dq_v2.log). Needs a block count divisible by 8; identity
// otherwise. Which block computes what changes, no result does.
DEVINL void xcd_block_index(int& bx, int& by, int& bz) {
  const unsigned nx = gridDim.x, ny = gridDim.y;
  const unsigned n = nx * ny * gridDim.z;
  unsigned l = blockIdx.x + nx * (blockIdx.y + ny * blockIdx.z);
  if (n % 8 == 0) l = (l % 8) * (n / 8) + l / 8;
  bx = l % nx;
  l /= nx;
  by = l % ny;
  bz = l / ny;
}

// ---- two-phase tile staging (async-STAGE split) -----------------------
// A [64][D] bf16 tile staged by all 512 threads: issue() starts the
// global loads into registers; write_rm()/write_tr() put them into LDS
// (row-major swizzled / transposed swizzled). OOB rows load zero.
template <int D, int NTH = NTHREADS>
struct TileStage {
  static constexpr int VPR = D / 8;              // 16B vecs per row
  static constexpr int VPT = 64 * VPR / NTH;     // vecs per thread
  uint4 vals[VPT];

  DEVINL void issue(const bf16_t* src, long row0, long row_limit,
                    long tok_stride) {
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int vi = threadIdx.x + i * NTH;
      const int row = vi / VPR, cv = vi % VPR;
      uint4 val = {0, 0, 0, 0};
      if (row0 + row < row_limit)
        val = *(const uint4*)(src + (row0 + row) * tok_stride + cv * 8);
      vals[i] = val;
    }
  }

  DEVINL void write_rm(char* lds) const {
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int vi = threadIdx.x + i * NTH;
      const int row = vi / VPR, cv = vi % VPR;
      *(uint4*)(lds + swz_off(row, D * 2, cv * 16)) = vals[i];
    }
  }

};

// Loads a [D][64] tile (rows = d, cols = 64 tokens) from a
// pre-transposed [D][S_pad] plane (transpose.hip) into swizzled LDS with
// plain b128 writes — replaces the in-kernel scalar transpose scatter
// that measured ~20 LDS bank-conflict cycles per MFMA.
template <int D, int NTH = NTHREADS>
struct TileStageT {
  static constexpr int VPR = 64 / 8;
  static constexpr int VPT = D * VPR / NTH;
  uint4 vals[VPT];

  DEVINL void issue(const bf16_t* plane, int col0, long S_pad) {
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int vi = threadIdx.x + i * NTH;
      const int row = vi / VPR, cv = vi % VPR;
      vals[i] = *(const uint4*)(plane + (long)row * S_pad + col0 + cv * 8);
    }
  }

  DEVINL void write(char* lds) const {
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int vi = threadIdx.x + i * NTH;
      const int row = vi / VPR, cv = vi % VPR;
      *(uint4*)(lds + swz_off(row, 128, cv * 16)) = vals[i];
    }
  }
};

// B-fragment read from a swizzled row-major LDS tile, row stride RB bytes.
template <int RB>
DEVINL bf16x8v read_bfrag(const char* lds, int row, int col_elem) {
  return as_frag(*(const uint4*)(lds + swz_off(row, RB, col_elem * 2)));
}

// A-fragment set (rows m = lane&15 of a 16-row strip) from global.
template <int D>
DEVINL void load_afrags(bf16x8v* frag, const bf16_t* src, long row,
                        long row_limit, long tok_stride, int lane) {
  constexpr int DC = D / 32;
#pragma unroll
  for (int c = 0; c < DC; ++c) {
    uint4 raw = {0, 0, 0, 0};
    if (row < row_limit)
      raw = *(const uint4*)(src + row * tok_stride + c * 32 + (lane >> 4) * 8);
    frag[c] = as_frag(raw);
  }
}

// ========================================================================
// Forward v3: grid (ceil(S/256), Hq, B); block = 8 waves, wave = 32 q rows.
//
// Swapped QK^T on mfma_f32_32x32x16_bf16: compute S^T = K·Q^T so each
// lane owns ONE q row (lane&31) and its P values stay in-register —
// row reduce is an in-lane chain + one half-wave exchange; no P LDS
// round trip. P is repacked to the PV A-fragment layout with
// v_cvt_pk_bf16_f32 pairs + permlane32_swap (guide T12):
//   C-layout kv of reg r (half h): (r&3) + 8*(r>>2) + 4*h
//   A-layout needs kv = h*8 + j in each 16-slot; one swap fixes two words.
// Q lives in registers as the MFMA B-operand (B[k][n]: n = lane&31 = its
// q row, k contiguous per half) — loaded once per wave.
// ========================================================================
using f32x16 = __attribute__((ext_vector_type(16))) float;

using f32x2 = __attribute__((ext_vector_type(2))) float;
using bf16x2v = __attribute__((ext_vector_type(2))) __bf16;

// Two floats -> one word of two bf16 (lo in bits 0..15). The vector convert
// is ONE v_cvt_pk_bf16_f32 with the hardware's round-to-nearest-even; two
// scalar __float2bfloat16 plus a shift and an or compiled to four
// instructions per pair for the same bits.
DEVINL uint32_t pack_bf16(float lo, float hi) {
  const f32x2 f = {lo, hi};
  union { bf16x2v b; uint32_t u; } c;
  c.b = __builtin_convertvector(f, bf16x2v);
  return c.u;
}

// One 32x32 f32 C-layout strip (P^T or dS^T) -> the next MFMA's two bf16
// A-fragments: cvt_pk pairs + permlane32_swap (guide T12).
DEVINL void repack_pa(const f32x16& pt, bf16x8v& pa0, bf16x8v& pa1) {
  union { uint32_t w[4]; bf16x8v f; } f0, f1;
  auto sA = __builtin_amdgcn_permlane32_swap(
      pack_bf16(pt[0], pt[1]), pack_bf16(pt[4], pt[5]), false, false);
  auto sB = __builtin_amdgcn_permlane32_swap(
      pack_bf16(pt[2], pt[3]), pack_bf16(pt[6], pt[7]), false, false);
  f0.w[0] = sA[0]; f0.w[1] = sB[0]; f0.w[2] = sA[1]; f0.w[3] = sB[1];
  auto sC = __builtin_amdgcn_permlane32_swap(
      pack_bf16(pt[8], pt[9]), pack_bf16(pt[12], pt[13]), false, false);
  auto sD = __builtin_amdgcn_permlane32_swap(
      pack_bf16(pt[10], pt[11]), pack_bf16(pt[14], pt[15]), false, false);
  f1.w[0] = sC[0]; f1.w[1] = sD[0]; f1.w[2] = sC[1]; f1.w[3] = sD[1];
  pa0 = f0.f;
  pa1 = f1.f;
}

template <int D, bool CAUSAL>
__global__ __launch_bounds__(NTHREADS) void attn_fwd_kernel_v3(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ vt, bf16_t* __restrict__ o,
    float* __restrict__ lse, int B, int S, int Hq, int Hkv, int S_pad,
    float scale) {
  constexpr int QC = D / 16;    // Q B-fragments (k-slots of 16)
  constexpr int DT = D / 32;    // O col tiles of 32
  constexpr int BM3 = NW * 32;  // 256 q rows per block
  constexpr int KB = BN * D * 2;
  // double-buffered K|VT: one barrier per tile; tile t+1's LDS write
  // overlaps other waves' compute on tile t
  __shared__ __attribute__((aligned(16))) char smem[2 * (2 * KB)];

  const int lane = threadIdx.x & 63;
  const int hi = lane >> 5;
  const int wid = threadIdx.x >> 6;
  const int m0 = blockIdx.x * BM3;
  const int m0w = m0 + wid * 32;
  const int hq = blockIdx.y;
  const int b = blockIdx.z;
  const int hkv = hq / (Hq / Hkv);

  const long q_tok = (long)Hq * D, kv_tok = (long)Hkv * D;
  const bf16_t* qp = q + ((long)b * S * q_tok) + (long)hq * D;
  const bf16_t* kp = k + ((long)b * S * kv_tok) + (long)hkv * D;
  const bf16_t* vtp = vt + ((long)b * Hkv + hkv) * D * (long)S_pad;
  bf16_t* op = o + ((long)b * S * q_tok) + (long)hq * D;
  float* lsep = lse + ((long)b * Hq + hq) * S;

  const int qrow = m0w + (lane & 31);
  bf16x8v q_reg[QC];
#pragma unroll
  for (int c = 0; c < QC; ++c) {
    uint4 raw = {0, 0, 0, 0};
    if (qrow < S)
      raw = *(const uint4*)(qp + (long)qrow * q_tok + c * 16 + hi * 8);
    q_reg[c] = as_frag(raw);
  }

  f32x16 o_acc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[t][r] = 0.f;
  float m_run = NEG_INF, l_run = 0.f;

  TileStage<D> k_st;
  TileStageT<D> v_st;
  const int n_end = CAUSAL ? min(S, m0 + BM3) : S;
  k_st.issue(kp, 0, S, kv_tok);
  v_st.issue(vtp, 0, S_pad);
  k_st.write_rm(smem);
  v_st.write(smem + KB);
  __syncthreads();
  int cur = 0;

  for (int n0 = 0; n0 < n_end; n0 += BN) {
    char* k_lds = smem + cur * (2 * KB);
    char* vt_lds = k_lds + KB;
    const bool more = n0 + BN < n_end;
    if (more) {
      k_st.issue(kp, n0 + BN, S, kv_tok);
      v_st.issue(vtp, n0 + BN, S_pad);
    }

    const bool strip_live = !CAUSAL || (n0 <= m0w + 31);
    if (strip_live) {
      // S^T strips (two 32-kv subtiles x 32 q cols)
      f32x16 st[2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int r = 0; r < 16; ++r) st[ks][r] = 0.f;
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int c = 0; c < QC; ++c) {
          bf16x8v ka = read_bfrag<D * 2>(
              k_lds, ks * 32 + (lane & 31), c * 16 + hi * 8);
          st[ks] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              ka, q_reg[c], st[ks], 0, 0, 0);
        }
      __builtin_amdgcn_s_setprio(0);

      // mask + scale + in-lane row max; interior tiles (fully below the
      // diagonal and inside S) skip the per-element mask entirely
      const bool needs_mask = (n0 + BN > S) ||
                              (CAUSAL && (n0 + BN - 1 > m0w));
      float mx = NEG_INF;
      if (needs_mask) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kvg = n0 + ks * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            float s = st[ks][r] * scale;
            if ((CAUSAL && kvg > qrow) || kvg >= S || qrow >= S) s = NEG_INF;
            st[ks][r] = s;
            mx = fmaxf(mx, s);
          }
      } else {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float s = st[ks][r] * scale;
            st[ks][r] = s;
            mx = fmaxf(mx, s);
          }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      // defer-max (guide T13): when every row's max grew by < THR keep
      // the old running max and skip the O rescale; P is then bounded by
      // e^THR which the fp32 accumulator tolerates. Nothing of this tile
      // is pending when the branch is taken (P*V of tile t completes
      // before tile t+1's decision), so the T13 ordering hazard cannot
      // occur in this structure.
      constexpr float DEFER_THR = 8.f;
      const bool rescale = !__all(mx <= m_run + DEFER_THR);
      float alpha = 1.f;
      if (rescale) {
        const float mn = fmaxf(m_run, mx);
        alpha = (m_run == NEG_INF) ? 0.f : __expf(m_run - mn);
        m_run = mn;
      }
      float rsum = 0.f;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pe =
              (st[ks][r] == NEG_INF) ? 0.f : __expf(st[ks][r] - m_run);
          st[ks][r] = pe;
          rsum += pe;
        }
      rsum += __shfl_xor(rsum, 32, 64);
      l_run = l_run * alpha + rsum;

      // rescale O by the per-ROW alpha (rows are reg-mapped; alpha is
      // lane-mapped -> one bpermute gather per reg row); skipped
      // entirely on the defer path
      if (rescale) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rowidx = (r & 3) + 8 * (r >> 2) + 4 * hi;
          const float ar = __shfl(alpha, rowidx, 64);
#pragma unroll
          for (int t = 0; t < DT; ++t) o_acc[t][r] *= ar;
        }
      }

      // P (f32, C-layout) -> bf16 A-fragments via cvt_pk + permlane swap
      bf16x8v pa[4];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        union { uint32_t w[4]; bf16x8v f; } f0, f1;
        {
          auto sA = __builtin_amdgcn_permlane32_swap(
              pack_bf16(st[ks][0], st[ks][1]),
              pack_bf16(st[ks][4], st[ks][5]), false, false);
          auto sB = __builtin_amdgcn_permlane32_swap(
              pack_bf16(st[ks][2], st[ks][3]),
              pack_bf16(st[ks][6], st[ks][7]), false, false);
          f0.w[0] = sA[0]; f0.w[1] = sB[0]; f0.w[2] = sA[1]; f0.w[3] = sB[1];
        }
        {
          auto sC = __builtin_amdgcn_permlane32_swap(
              pack_bf16(st[ks][8], st[ks][9]),
              pack_bf16(st[ks][12], st[ks][13]), false, false);
          auto sD = __builtin_amdgcn_permlane32_swap(
              pack_bf16(st[ks][10], st[ks][11]),
              pack_bf16(st[ks][14], st[ks][15]), false, false);
          f1.w[0] = sC[0]; f1.w[1] = sD[0]; f1.w[2] = sC[1]; f1.w[3] = sD[1];
        }
        pa[2 * ks] = f0.f;
        pa[2 * ks + 1] = f1.f;
      }

      // O += P * V
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int t = 0; t < DT; ++t) {
          bf16x8v vb = read_bfrag<128>(
              vt_lds, t * 32 + (lane & 31), ks * 16 + hi * 8);
          o_acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              pa[ks], vb, o_acc[t], 0, 0, 0);
        }
      __builtin_amdgcn_s_setprio(0);
    }
    if (more) {
      char* nk = smem + (cur ^ 1) * (2 * KB);
      k_st.write_rm(nk);
      v_st.write(nk + KB);
    }
    __syncthreads();
    cur ^= 1;
  }

  // epilogue: O = o_acc / l (per reg row); LSE per lane row
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rowidx = (r & 3) + 8 * (r >> 2) + 4 * hi;
    const float lv = __shfl(l_run, rowidx, 64);
    const float inv_l = (lv > 0.f) ? 1.f / lv : 0.f;
    const int row = m0w + rowidx;
    if (row >= S) continue;
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const int col = t * 32 + (lane & 31);
      op[(long)row * q_tok + col] = f2bf(o_acc[t][r] * inv_l);
    }
  }
  if (hi == 0 && qrow < S)
    lsep[qrow] = (l_run > 0.f) ? m_run + __logf(l_run) : NEG_INF;
}

// ========================================================================
// Forward v4 (tok_attn_fwd variant 0, the default): v3's structure with
// less vector work around the same 32 MFMAs per tile.
//  * The running max m_run is kept in log2 units of the SCALED score, so a
//    probability is exp2(fma(s, scale*log2e, -m_run)): one v_fma and one
//    v_exp per score where v3 spends a multiply, a subtract, the multiply
//    inside __expf and the v_exp. The row max is taken over the raw MFMA
//    output (scale > 0 keeps the order) and scaled once per lane.
//  * No per-score `== -inf ? 0` select: a masked score is -inf, the fma
//    keeps it -inf and exp2(-inf) is 0. Only a running max that is still
//    -inf (a row that has seen no key yet: rows >= S) would give
//    -inf - -inf; it is replaced by 0 once per lane per tile.
//  * K fragments are read ahead of their MFMAs: the first 32-key half's 8
//    ds_read_b128 are all in flight before its chain and the second half's
//    are issued one per MFMA of the first (sched_group_barrier); left to
//    itself the compiler reads one fragment ahead with a wait per MFMA.
//  * Epilogue: O leaves through the block's own LDS (K|V^T are dead after
//    the loop's last barrier; 8 waves x 32 rows x 2D bytes is exactly the
//    double buffer) as whole rows in 16-byte stores; v3 writes 64 two-byte
//    stores per lane at a row stride. 1/l comes back reg-mapped from four
//    b128 reads of a 128-byte LDS copy instead of 16 bpermutes.
// ========================================================================
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

// Document bounds of a wave's 32 q rows (packed-document training): query i
// sees key j iff doc_start[b, i] <= j <= i. The forward and dQ kernels own
// one q row per lane, so the bound is one register next to q_reg.
//  * dstart: this lane's bound, clamped into [0, row]. Rows past S take
//    row S-1's, so the wave's last lane still holds the largest bound.
//  * wave_min / wave_max: the bounds of the wave's first and last row
//    (doc_start is non-decreasing), wave-uniform. A tile that ends at or
//    before wave_min is dead for the whole wave; a tile that begins before
//    wave_max needs the per-element mask.
//  * n_begin: first key tile of the block, the tile of row m0's bound,
//    clamped into [0, tile of m0].
// Nothing here is trusted: every value derived from the tensor is clamped
// into the range the plain causal kernel touches, so a malformed tensor
// gives wrong numbers and no out-of-range access.
//
// The kernels take the [B, S] tensor as a trailing parameter pack: one
// `const int*` with DOC, empty without, so the plain instantiations keep
// their argument list. Their DocRows is the specialisation below whose
// members are compile-time zeros: with run-time zeros the D = 64 kernels
// came out four VGPRs larger, though every use folds away in the end.
DEVINL const int* first_arg(const int* p) { return p; }

template <bool DOC>
struct DocRows {
  int dstart, wave_min, wave_max, n_begin;
  DEVINL DocRows(int b, int S, int m0, int qrow, const int* doc_start) {
    const int* dsp = doc_start + (long)b * S;
    const int row = min(qrow, S - 1);
    dstart = max(0, min(dsp[row], row));
    wave_min = __builtin_amdgcn_readfirstlane(dstart);
    wave_max = __builtin_amdgcn_readlane(dstart, 31);
    n_begin = max(0, min(dsp[m0], m0)) / BN * BN;
  }
};

template <>
struct DocRows<false> {
  static constexpr int dstart = 0, wave_min = 0, wave_max = 0, n_begin = 0;
  DEVINL DocRows(int, int, int, int) {}
};

template <int D, bool CAUSAL, bool DOC = false, typename... DOCARG>
__global__ __launch_bounds__(NTHREADS) void attn_fwd_kernel_v4(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ vt, bf16_t* __restrict__ o,
    float* __restrict__ lse, int B, int S, int Hq, int Hkv, int S_pad,
    float scale, DOCARG... doc_start) {
  static_assert(!DOC || CAUSAL, "document bounds refine the causal mask");
  static_assert(sizeof...(DOCARG) == (DOC ? 1 : 0), "one tensor with DOC");
  constexpr int QC = D / 16;    // Q B-fragments (k-slots of 16)
  constexpr int DT = D / 32;    // O col tiles of 32
  constexpr int BM3 = NW * 32;  // 256 q rows per block
  constexpr int KB = BN * D * 2;
  constexpr int OWB = 32 * D * 2;   // a wave's O rows in the epilogue
  static_assert(NW * OWB <= 2 * (2 * KB), "O staging fits the K|VT buffers");
  __shared__ __attribute__((aligned(16))) char smem[2 * (2 * KB)];

  const int lane = threadIdx.x & 63;
  const int hi = lane >> 5;
  const int wid = threadIdx.x >> 6;
  int bx, hq, b;
  xcd_block_index(bx, hq, b);
  const int m0 = bx * BM3;
  const int m0w = m0 + wid * 32;
  const int hkv = hq / (Hq / Hkv);

  const long q_tok = (long)Hq * D, kv_tok = (long)Hkv * D;
  const bf16_t* qp = q + ((long)b * S * q_tok) + (long)hq * D;
  const bf16_t* kp = k + ((long)b * S * kv_tok) + (long)hkv * D;
  const bf16_t* vtp = vt + ((long)b * Hkv + hkv) * D * (long)S_pad;
  bf16_t* op = o + ((long)b * S * q_tok) + (long)hq * D;
  float* lsep = lse + ((long)b * Hq + hq) * S;

  const int qrow = m0w + (lane & 31);
  bf16x8v q_reg[QC];
#pragma unroll
  for (int c = 0; c < QC; ++c) {
    uint4 raw = {0, 0, 0, 0};
    if (qrow < S)
      raw = *(const uint4*)(qp + (long)qrow * q_tok + c * 16 + hi * 8);
    q_reg[c] = as_frag(raw);
  }

  f32x16 o_acc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[t][r] = 0.f;
  // m_run: running row max of score*scale*log2e (log2 units)
  float m_run = NEG_INF, l_run = 0.f;
  const float c2 = scale * LOG2E;
  const DocRows<DOC> doc(b, S, m0, qrow, doc_start...);

  TileStage<D> k_st;
  TileStageT<D> v_st;
  const int n_end = CAUSAL ? min(S, m0 + BM3) : S;
  k_st.issue(kp, doc.n_begin, S, kv_tok);
  v_st.issue(vtp, doc.n_begin, S_pad);
  k_st.write_rm(smem);
  v_st.write(smem + KB);
  __syncthreads();
  int cur = 0;

  for (int n0 = doc.n_begin; n0 < n_end; n0 += BN) {
    char* k_lds = smem + cur * (2 * KB);
    char* vt_lds = k_lds + KB;
    const bool more = n0 + BN < n_end;
    if (more) {
      k_st.issue(kp, n0 + BN, S, kv_tok);
      v_st.issue(vtp, n0 + BN, S_pad);
    }

    const bool strip_live = (!CAUSAL || (n0 <= m0w + 31)) &&
                            (!DOC || n0 + BN > doc.wave_min);
    if (strip_live) {
      // S^T strips (two 32-kv subtiles x 32 q cols), raw (unscaled)
      f32x16 st[2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int r = 0; r < 16; ++r) st[ks][r] = 0.f;
      __builtin_amdgcn_s_setprio(1);
      // the first 32-key half's fragments are all in flight before its
      // MFMA chain; the second half's are read one per MFMA of the first
      bf16x8v ka[2][QC];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int c = 0; c < QC; ++c)
          ka[ks][c] = read_bfrag<D * 2>(
              k_lds, ks * 32 + (lane & 31), c * 16 + hi * 8);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int c = 0; c < QC; ++c)
          st[ks] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              ka[ks][c], q_reg[c], st[ks], 0, 0, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, QC, 0);
#pragma unroll
      for (int c = 0; c < QC; ++c) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, QC, 0);
      __builtin_amdgcn_s_setprio(0);

      // mask (edge tiles only) + in-lane row max of the raw scores. With
      // document bounds a row can meet whole tiles of -inf before its
      // first live key; m_run stays -inf through them and the two guards
      // below (alpha = 0, neg_m = 0) keep p, l_run and O at exactly 0.
      const bool needs_mask = (n0 + BN > S) ||
                              (CAUSAL && (n0 + BN - 1 > m0w)) ||
                              (DOC && n0 < doc.wave_max);
      if (needs_mask) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kvg = n0 + ks * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if ((CAUSAL && kvg > qrow) || kvg >= S || qrow >= S ||
                (DOC && kvg < doc.dstart))
              st[ks][r] = NEG_INF;
          }
      }
      float mx = NEG_INF;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[ks][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64)) * c2;
      // defer-max (guide T13): when every row's max grew by < THR keep
      // the old running max and skip the O rescale; P is then bounded by
      // e^THR which the fp32 accumulator tolerates. Nothing of this tile
      // is pending when the branch is taken (P*V of tile t completes
      // before tile t+1's decision), so the T13 ordering hazard cannot
      // occur in this structure. THR is 8 nats, in log2 units here.
      constexpr float DEFER_THR = 8.f * LOG2E;
      const bool rescale = !__all(mx <= m_run + DEFER_THR);
      float alpha = 1.f;
      if (rescale) {
        const float mn = fmaxf(m_run, mx);
        alpha = (m_run == NEG_INF) ? 0.f
                                   : __builtin_amdgcn_exp2f(m_run - mn);
        m_run = mn;
      }
      // a row with no live key so far: every score is -inf and must give
      // p = 0, not exp2(-inf + inf)
      const float neg_m = (m_run == NEG_INF) ? 0.f : -m_run;
      float rsum = 0.f;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pe =
              __builtin_amdgcn_exp2f(__builtin_fmaf(st[ks][r], c2, neg_m));
          st[ks][r] = pe;
          rsum += pe;
        }
      rsum += __shfl_xor(rsum, 32, 64);
      l_run = l_run * alpha + rsum;

      // rescale O by the per-ROW alpha (rows are reg-mapped; alpha is
      // lane-mapped -> one bpermute gather per reg row); skipped
      // entirely on the defer path
      if (rescale) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rowidx = (r & 3) + 8 * (r >> 2) + 4 * hi;
          const float ar = __shfl(alpha, rowidx, 64);
#pragma unroll
          for (int t = 0; t < DT; ++t) o_acc[t][r] *= ar;
        }
      }

      // P (f32, C-layout) -> bf16 A-fragments via cvt_pk + permlane swap
      bf16x8v pa[4];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        repack_pa(st[ks], pa[2 * ks], pa[2 * ks + 1]);

      // O += P * V
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int t = 0; t < DT; ++t) {
          bf16x8v vb = read_bfrag<128>(
              vt_lds, t * 32 + (lane & 31), ks * 16 + hi * 8);
          o_acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              pa[ks], vb, o_acc[t], 0, 0, 0);
        }
      __builtin_amdgcn_s_setprio(0);
    }
    if (more) {
      char* nk = smem + (cur ^ 1) * (2 * KB);
      k_st.write_rm(nk);
      v_st.write(nk + KB);
    }
    __syncthreads();
    cur ^= 1;
  }

  // epilogue. Every wave is past the loop's last barrier, so no K|V^T tile
  // is read any more and each wave owns OWB bytes of smem. Within a wave
  // LDS operations complete in program order.
  char* ow = smem + wid * OWB;
  if (hi == 0)
    *(float*)(ow + (lane & 31) * 4) = (l_run > 0.f) ? 1.f / l_run : 0.f;
  // 1/l of reg row r = 4g+j is row 8g + 4hi + j: four runs of four
  f32x4 il[4];
#pragma unroll
  for (int g = 0; g < 4; ++g)
    il[g] = *(const f32x4*)(ow + (8 * g + 4 * hi) * 4);
  __builtin_amdgcn_wave_barrier();
  // O^T fragments -> row-major bf16 rows. The two half-waves write rows 4
  // apart (same banks); XOR-ing byte 64 of the column with the row's bit 2
  // (= hi) puts them on disjoint banks.
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rowidx = (r & 3) + 8 * (r >> 2) + 4 * hi;
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const int cb = (t * 32 + (lane & 31)) * 2;
      *(bf16_t*)(ow + rowidx * (D * 2) + (cb ^ (hi << 6))) =
          f2bf(o_acc[t][r] * il[r >> 2][r & 3]);
    }
  }
  __builtin_amdgcn_wave_barrier();
  constexpr int CPR = D * 2 / 16;   // 16-byte chunks per row
  constexpr int RPI = WAVE / CPR;   // rows per wave-wide store
#pragma unroll
  for (int i = 0; i < 32 / RPI; ++i) {
    const int row = i * RPI + lane / CPR;
    const int ch = lane % CPR;
    const uint4 val = *(const uint4*)(
        ow + row * (D * 2) + ((ch * 16) ^ (((row >> 2) & 1) << 6)));
    if (m0w + row < S)
      *(uint4*)(op + (long)(m0w + row) * q_tok + ch * 8) = val;
  }
  if (hi == 0 && qrow < S)
    lsep[qrow] = (l_run > 0.f) ? m_run * LN2 + __logf(l_run) : NEG_INF;
}

// ========================================================================
// Backward preprocess: Dsum[b,h,m] = sum_d dO*O (fp32)
// ========================================================================
// grid (ceil(S/PRE_ROWS), Hq, B), 256 threads. A group of D/8 lanes
// covers one row with one uint4 each of dO and O (a 2*D-byte contiguous
// read per row) and reduces with xor-shuffles inside the group; the
// earlier one-thread-per-row form put neighbouring lanes 2*D bytes apart
// and ran at 0.9 TB/s. A wave walks 16 consecutive s of one head, so its
// 16 Dsum values leave as one contiguous 64-byte store. It also writes
// the fused dK+dV kernel's accumulator start values (rc, see there).
constexpr int PRE_ROWS = 64;   // s rows per block (16 per wave)

template <int D>
__global__ __launch_bounds__(256) void attn_bwd_pre_kernel(
    const bf16_t* __restrict__ dout, const bf16_t* __restrict__ o,
    const float* __restrict__ lse, float* __restrict__ dsum,
    float* __restrict__ rc, int Hq, int S, int S_pad, float sqrt_d) {
  constexpr int GL = D / 8;        // lanes per row
  constexpr int RPI = WAVE / GL;   // rows per wave per pass
  constexpr int NP = 16 / RPI;     // passes per wave
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int grp = lane / GL, gl = lane % GL;
  const int h = blockIdx.y;
  const long b = blockIdx.z;
  const int s0 = blockIdx.x * PRE_ROWS + wid * 16;
  const long tok = (long)Hq * D;
  const bf16_t* dp = dout + (b * S) * tok + (long)h * D + gl * 8;
  const bf16_t* op = o + (b * S) * tok + (long)h * D + gl * 8;

  uint4 av[NP], bv[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int s = s0 + p * RPI + grp;
    av[p] = bv[p] = uint4{0, 0, 0, 0};
    if (s < S) {
      av[p] = *(const uint4*)(dp + (long)s * tok);
      bv[p] = *(const uint4*)(op + (long)s * tok);
    }
  }
  // lane i (< 16) of the wave ends up holding row s0+i
  float mine = 0.f;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const uint16_t* ah = (const uint16_t*)&av[p];
    const uint16_t* bh = (const uint16_t*)&bv[p];
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      acc = fmaf(bfbits2f(ah[j]), bfbits2f(bh[j]), acc);
#pragma unroll
    for (int off = GL / 2; off > 0; off >>= 1)
      acc += __shfl_xor(acc, off, WAVE);
    // row p*RPI + g sits in every lane of group g; collect it in lane
    // (p*RPI + g) with one gather per pass
#pragma unroll
    for (int g = 0; g < RPI; ++g) {
      const float vg = __shfl(acc, g * GL, WAVE);
      if (lane == p * RPI + g) mine = vg;
    }
  }
  if (lane < 16) {
    const int s = s0 + lane;
    if (s < S) dsum[(b * Hq + h) * S + s] = mine;
    // start values of the fused dK+dV kernel's S and dP accumulators,
    // [B,Hq,2,S_pad]: -lse*sqrt(D) (or -1e30: p == 0 exactly, for padded
    // and lse == -inf rows) and -Dsum (0 for padded rows)
    if (s < S_pad) {
      float* r = rc + (b * Hq + h) * 2 * S_pad;
      const float l = (s < S) ? lse[(b * Hq + h) * S + s] : NEG_INF;
      r[s] = (l == NEG_INF) ? -1e30f : -l * sqrt_d;
      r[S_pad + s] = (s < S) ? -mine : 0.f;
    }
  }
}

// ========================================================================
// Backward dV / dK v3, SPLIT form: two kernels, grid (ceil(S/256), Hkv,
// B), 8 waves, wave = 32 kv rows. Splitting dV and dK keeps each kernel
// at 2 waves/SIMD; a combined kernel at 32 keys/wave needs dk+dv
// accumulators = 128 regs, drops to 1 wave/SIMD with nothing to fill the
// MFMA latency, and measured SLOWER than the 16x16 v2. The 64-keys-per-
// wave combined kernel (attn_bwd_dkdv_kernel below) is the case that
// conclusion left out: it accepts 1 wave/SIMD and gets its latency hiding
// from two independent 32-key chains per wave. The split pair stays
// selectable (tok_attn_bwd's `split` argument) so both can be timed in
// one process. Swapped-operand structure as the forward: K lives in
// registers as the MFMA B-operand; P^T / dS^T stay in-register and are
// repacked with cvt_pk+permlane32_swap.
// ========================================================================
template <int D, bool CAUSAL>
__global__ __launch_bounds__(NTHREADS) void attn_bwd_dv_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ dot_t, const bf16_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ dsum,
    bf16_t* __restrict__ dv, int B, int S, int Hq, int Hkv, int S_pad,
    float scale) {
  constexpr int QC = D / 16;
  constexpr int DT = D / 32;
  constexpr int NTH = NTHREADS;
  constexpr int BNK = NW * 32;  // kv rows per block
  constexpr int KB = BN * D * 2;
  // double-buffered (Q rm | dOT): one barrier per q tile
  __shared__ __attribute__((aligned(16))) char smem[2 * (2 * KB)];

  const int lane = threadIdx.x & 63;
  const int hi = lane >> 5;
  const int wid = threadIdx.x >> 6;
  const int n0 = blockIdx.x * BNK;
  const int n0w = n0 + wid * 32;
  const int hkv = blockIdx.y;
  const int b = blockIdx.z;
  const int rep = Hq / Hkv;

  const long q_tok = (long)Hq * D, kv_tok = (long)Hkv * D;
  const bf16_t* kp = k + ((long)b * S * kv_tok) + (long)hkv * D;
  bf16_t* dvp = dv + ((long)b * S * kv_tok) + (long)hkv * D;

  const int kvrow = n0w + (lane & 31);
  bf16x8v k_reg[QC];
#pragma unroll
  for (int c = 0; c < QC; ++c) {
    uint4 kr = {0, 0, 0, 0};
    if (kvrow < S)
      kr = *(const uint4*)(kp + (long)kvrow * kv_tok + c * 16 + hi * 8);
    k_reg[c] = as_frag(kr);
  }

  f32x16 dv_acc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) dv_acc[t][r] = 0.f;

  const int m_start = CAUSAL ? (n0 / BN) * BN : 0;
  const long dplane = (long)D * S_pad;
  TileStage<D, NTH> q_st;
  TileStageT<D, NTH> do_st;
  const bf16_t* dot0 = dot_t + ((long)b * Hq + hkv * rep) * dplane;
  q_st.issue(q + ((long)b * S * q_tok) + (long)(hkv * rep) * D, m_start, S,
             q_tok);
  do_st.issue(dot0, m_start, S_pad);
  q_st.write_rm(smem);
  do_st.write(smem + KB);
  __syncthreads();
  int cur = 0;

  for (int g = 0; g < rep; ++g) {
    const int hq = hkv * rep + g;
    const bf16_t* qp = q + ((long)b * S * q_tok) + (long)hq * D;
    const bf16_t* dotp = dot_t + ((long)b * Hq + hq) * dplane;
    const float* lsep = lse + ((long)b * Hq + hq) * S;

    for (int m0 = m_start; m0 < S; m0 += BN) {
      char* q_lds = smem + cur * (2 * KB);
      char* dot_lds = q_lds + KB;
      const int m1 = m0 + BN;
      const bool more = m1 < S || g + 1 < rep;
      if (m1 < S) {
        q_st.issue(qp, m1, S, q_tok);
        do_st.issue(dotp, m1, S_pad);
      } else if (g + 1 < rep) {
        q_st.issue(qp + D, m_start, S, q_tok);
        do_st.issue(dotp + dplane, m_start, S_pad);
      }

#pragma unroll
      for (int qs = 0; qs < 2; ++qs) {
        f32x16 sv;
#pragma unroll
        for (int r = 0; r < 16; ++r) sv[r] = 0.f;
#pragma unroll
        for (int c = 0; c < QC; ++c) {
          bf16x8v qa = read_bfrag<D * 2>(
              q_lds, qs * 32 + (lane & 31), c * 16 + hi * 8);
          sv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              qa, k_reg[c], sv, 0, 0, 0);
        }
        const int qg_lane = m0 + qs * 32 + (lane & 31);
        const float lse_lane = (qg_lane < S) ? lsep[qg_lane] : NEG_INF;
        f32x16 pt;
        // interior subtile: all q rows >= every kv row of the wave and
        // in-bounds -> the per-element mask chain is dead VALU work
        // (PMC r2: bwd is ~11 VALU/MFMA). One loop, uniform flag: the
        // exp stays common so the compiler shares registers.
        const bool need_mask = (CAUSAL && m0 + qs * 32 < n0w + 32) ||
                               (m0 + qs * 32 + 32 > S) || (n0w + 32 > S);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rowidx = (r & 3) + 8 * (r >> 2) + 4 * hi;
          const float lse_r = __shfl(lse_lane, rowidx, 64);
          float pv = __expf(sv[r] * scale - lse_r);
          if (need_mask) {
            const int qg = m0 + qs * 32 + rowidx;
            if (!(qg < S && kvrow < S && (!CAUSAL || qg >= kvrow) &&
                  lse_r != NEG_INF))
              pv = 0.f;
          }
          pt[r] = pv;
        }
        bf16x8v pa0, pa1;
        repack_pa(pt, pa0, pa1);
#pragma unroll
        for (int t = 0; t < DT; ++t) {
          bf16x8v b0 = read_bfrag<128>(
              dot_lds, t * 32 + (lane & 31), qs * 32 + hi * 8);
          dv_acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              pa0, b0, dv_acc[t], 0, 0, 0);
          bf16x8v b1 = read_bfrag<128>(
              dot_lds, t * 32 + (lane & 31), qs * 32 + 16 + hi * 8);
          dv_acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              pa1, b1, dv_acc[t], 0, 0, 0);
        }
      }
      if (more) {
        char* nq = smem + (cur ^ 1) * (2 * KB);
        q_st.write_rm(nq);
        do_st.write(nq + KB);
      }
      __syncthreads();
      cur ^= 1;
    }
  }

#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = n0w + (r & 3) + 8 * (r >> 2) + 4 * hi;
    if (row >= S) continue;
#pragma unroll
    for (int t = 0; t < DT; ++t)
      dvp[(long)row * kv_tok + t * 32 + (lane & 31)] = f2bf(dv_acc[t][r]);
  }
}

template <int D, bool CAUSAL>
__global__ __launch_bounds__(NTHREADS) void attn_bwd_dk_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ v, const bf16_t* __restrict__ dout,
    const bf16_t* __restrict__ q_t, const float* __restrict__ lse,
    const float* __restrict__ dsum, bf16_t* __restrict__ dk, int B, int S,
    int Hq, int Hkv, int S_pad, float scale) {
  constexpr int QC = D / 16;
  constexpr int DT = D / 32;
  constexpr int NTH = NTHREADS;
  constexpr int BNK = NW * 32;
  constexpr int KB = BN * D * 2;
  // Q rm | QT | dO rm | V block tile (staged once; keeping V in
  // registers alongside K pushed the kernel to 256 VGPR + scratch spill)
  __shared__ __attribute__((aligned(16))) char smem[3 * KB + BNK * D * 2];
  char* q_lds = smem;
  char* qt_lds = smem + KB;
  char* do_lds = smem + 2 * KB;
  char* v_lds = smem + 3 * KB;

  const int lane = threadIdx.x & 63;
  const int hi = lane >> 5;
  const int wid = threadIdx.x >> 6;
  const int n0 = blockIdx.x * BNK;
  const int n0w = n0 + wid * 32;
  const int hkv = blockIdx.y;
  const int b = blockIdx.z;
  const int rep = Hq / Hkv;

  const long q_tok = (long)Hq * D, kv_tok = (long)Hkv * D;
  const bf16_t* kp = k + ((long)b * S * kv_tok) + (long)hkv * D;
  const bf16_t* vp = v + ((long)b * S * kv_tok) + (long)hkv * D;
  bf16_t* dkp = dk + ((long)b * S * kv_tok) + (long)hkv * D;

  const int kvrow = n0w + (lane & 31);
  bf16x8v k_reg[QC];
#pragma unroll
  for (int c = 0; c < QC; ++c) {
    uint4 kr = {0, 0, 0, 0};
    if (kvrow < S)
      kr = *(const uint4*)(kp + (long)kvrow * kv_tok + c * 16 + hi * 8);
    k_reg[c] = as_frag(kr);
  }
  {  // stage the block's 256-row V tile (row-major, swizzled) once
    constexpr int VPR = D / 8;
#pragma unroll 4
    for (int vi = threadIdx.x; vi < BNK * VPR; vi += NTH) {
      const int row = vi / VPR, cv = vi % VPR;
      uint4 val = {0, 0, 0, 0};
      if (n0 + row < S)
        val = *(const uint4*)(vp + (long)(n0 + row) * kv_tok + cv * 8);
      *(uint4*)(v_lds + swz_off(row, D * 2, cv * 16)) = val;
    }
  }

  f32x16 dk_acc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) dk_acc[t][r] = 0.f;

  const int m_start = CAUSAL ? (n0 / BN) * BN : 0;

  for (int g = 0; g < rep; ++g) {
    const int hq = hkv * rep + g;
    const bf16_t* qp = q + ((long)b * S * q_tok) + (long)hq * D;
    const bf16_t* dop = dout + ((long)b * S * q_tok) + (long)hq * D;
    const float* lsep = lse + ((long)b * Hq + hq) * S;
    const float* dsp = dsum + ((long)b * Hq + hq) * S;

    const bf16_t* qtp = q_t + ((long)b * Hq + hq) * (long)D * S_pad;
    for (int m0 = m_start; m0 < S; m0 += BN) {
      {  // synchronous staging: the prefetch ring costs ~16 VGPRs and
         // tips this kernel into scratch spill, which is worse
        TileStage<D, NTH> q_st, do_st;
        TileStageT<D, NTH> qt_st;
        q_st.issue(qp, m0, S, q_tok);
        do_st.issue(dop, m0, S, q_tok);
        qt_st.issue(qtp, m0, S_pad);
        q_st.write_rm(q_lds);
        qt_st.write(qt_lds);
        do_st.write_rm(do_lds);
      }
      __syncthreads();

#pragma unroll
      for (int qs = 0; qs < 2; ++qs) {
        f32x16 sv, dpv;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          sv[r] = 0.f;
          dpv[r] = 0.f;
        }
#pragma unroll
        for (int c = 0; c < QC; ++c) {
          bf16x8v qa = read_bfrag<D * 2>(
              q_lds, qs * 32 + (lane & 31), c * 16 + hi * 8);
          sv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              qa, k_reg[c], sv, 0, 0, 0);
          bf16x8v doa = read_bfrag<D * 2>(
              do_lds, qs * 32 + (lane & 31), c * 16 + hi * 8);
          bf16x8v vb = read_bfrag<D * 2>(
              v_lds, wid * 32 + (lane & 31), c * 16 + hi * 8);
          dpv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              doa, vb, dpv, 0, 0, 0);
        }
        const int qg_lane = m0 + qs * 32 + (lane & 31);
        const float lse_lane = (qg_lane < S) ? lsep[qg_lane] : NEG_INF;
        const float ds_lane = (qg_lane < S) ? dsp[qg_lane] : 0.f;
        f32x16 dst;
        // interior fast path, one loop + uniform flag (see dv kernel)
        const bool need_mask = (CAUSAL && m0 + qs * 32 < n0w + 32) ||
                               (m0 + qs * 32 + 32 > S) || (n0w + 32 > S);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rowidx = (r & 3) + 8 * (r >> 2) + 4 * hi;
          const float lse_r = __shfl(lse_lane, rowidx, 64);
          const float ds_r = __shfl(ds_lane, rowidx, 64);
          float pv = __expf(sv[r] * scale - lse_r);
          if (need_mask) {
            const int qg = m0 + qs * 32 + rowidx;
            if (!(qg < S && kvrow < S && (!CAUSAL || qg >= kvrow) &&
                  lse_r != NEG_INF))
              pv = 0.f;
          }
          dst[r] = pv * (dpv[r] - ds_r);
        }
        bf16x8v da0, da1;
        repack_pa(dst, da0, da1);
#pragma unroll
        for (int t = 0; t < DT; ++t) {
          bf16x8v b0 = read_bfrag<128>(
              qt_lds, t * 32 + (lane & 31), qs * 32 + hi * 8);
          dk_acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              da0, b0, dk_acc[t], 0, 0, 0);
          bf16x8v b1 = read_bfrag<128>(
              qt_lds, t * 32 + (lane & 31), qs * 32 + 16 + hi * 8);
          dk_acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              da1, b1, dk_acc[t], 0, 0, 0);
        }
      }
      __syncthreads();
    }
  }

#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = n0w + (r & 3) + 8 * (r >> 2) + 4 * hi;
    if (row >= S) continue;
#pragma unroll
    for (int t = 0; t < DT; ++t)
      dkp[(long)row * kv_tok + t * 32 + (lane & 31)] =
          f2bf(dk_acc[t][r] * scale);
  }
}

// ========================================================================
// Backward dK+dV FUSED: grid (ceil(S/256), Hkv, B); 4 waves, 1 wave/SIMD,
// wave = 64 keys as two 32-key halves. S = Q·K^T, its exp and its mask are
// computed once for both outputs, and every Q/dO/Q^T/dO^T fragment read
// from LDS feeds two MFMAs (one per half); the two halves are independent
// MFMA chains, which is the latency hiding the second wave per SIMD gives
// the split kernels. dK^T and dV^T of the wave's 64 keys live in 256
// accumulator registers for the whole sweep over rep heads x q tiles.
//
// Row constants ride in the accumulators: S starts at -lse*sqrt(D) and dP
// at -Dsum, so p = exp2(S' * log2(e)/sqrt(D)) and dS = p * dP' need no
// per-element shuffle, subtract or row maximum. A row's start value
// depends only on (r, hi) - four runs of four consecutive rows - so it is
// 4 b128 reads per operand from a 256-byte LDS copy staged with the tile.
// The start values come ready-made from attn_bwd_pre_kernel ([B,Hq,2,
// S_pad]): padded q rows and lse == -inf rows hold S' = -1e30, so the
// exponent goes to -inf and p is exactly 0; only the key side (diagonal,
// keys >= S) still needs the per-element mask.
//
// LDS: a 64-row stage of the four images (Q rm, Q^T, dO rm, dO^T) is
// 64 KiB; double-buffered next to the block's 64 KiB V tile that is
// 192 KiB > 160 KiB. Way out taken: 32-ROW STAGES (2 x 32.25 KiB + 64 KiB
// V = 128.5 KiB). V in registers would cost 64 more VGPRs on top of
// dK 128 + dV 128 + K 64, and the kernel already sits at 512; the single
// dual-use image (tr-reads) needs an operand layout nothing here has
// verified on hardware. The pre-transposed Q^T/dO^T planes are kept.
//
// Staging: at 1 wave/SIMD nothing else covers a global load's latency, so
// the next stage must be in flight for a whole tile, and a register ring
// that deep (33 VGPRs) does not fit. The stage is loaded global -> LDS by
// DMA instead (DkdvStage): issued at the top of a tile into the idle
// buffer, retired with vmcnt(0) just before the tile's barrier. Measured
// on the whole backward at B=8 S=4096: register ring split in two halves
// 10.1 ms, DMA 9.4 ms (split dV/dK pair 12.9 ms); profiles/attn_dkdv.log.
// ========================================================================
constexpr int NW_KV = 4;              // waves per block in the fused kernel
constexpr int NTH_KV = NW_KV * WAVE;  // 256
constexpr int QROWS = 32;             // q rows per stage

// Inverse of swz_off: the (row, byte-in-row) whose swizzled offset is o.
DEVINL void unswz(int o, int row_bytes, int& row, int& byte_in_row) {
  const int k = 256 / row_bytes;   // rows per 256-byte XOR group
  const int base = (o >> 8) * k;
  row = base;
  byte_in_row = 0;
  for (int rl = 0; rl < k; ++rl) {
    const int r = base + rl;
    const int x = o ^ ((r & 15) << 4);
    if (x / row_bytes == r) {
      row = r;
      byte_in_row = x - r * row_bytes;
    }
  }
}

// BYTES-per-lane global -> LDS DMA: lane i's bytes land at
// lds_wave_base + BYTES*i. Inline asm, with M0 (the DMA's LDS base) saved
// and restored: the compiler then does not see an LDS write it would
// order every later ds_read behind with vmcnt(0); DkdvStage::finish()
// and the block barrier do that ordering instead.
template <int BYTES>
DEVINL void glds(const void* g, char* lds_wave_base) {
  static_assert(BYTES == 16 || BYTES == 4, "dwordx4 or dword");
  const uint32_t dst = __builtin_amdgcn_readfirstlane(
      (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)
          lds_wave_base);
  uint32_t keep;
  if (BYTES == 16)
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(g), "s"(dst)
        : "memory");
  else
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
        "global_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(g), "s"(dst)
        : "memory");
}

// One stage = the four [32 q rows] images + 64 row constants. The images
// go global -> LDS directly (global_load_lds_dwordx4, no staging
// registers: the kernel is at the register cap). A wave-instruction
// writes 64 x 16 B linearly, so the swizzle is applied on the SOURCE
// side: the lane that lands on LDS offset o loads the chunk whose
// swz_off is o. Rows past S re-read row S-1 (finite data; their P and dS
// are exactly 0 through the row constant) since a DMA cannot write
// zeros.
template <int D>
struct DkdvStage {
  static constexpr int VPR = D / 8;                 // 16B vecs per rm row
  static constexpr int NV = QROWS * VPR / NTH_KV;   // vecs/thread/image
  static constexpr int TB = QROWS * D * 2;          // bytes per image
  static constexpr int RC_OFF = 4 * TB;             // 32 S' + 32 dP' starts
  static constexpr int BYTES = 4 * TB + 256;
  // source of this lane's first chunk per image; chunk i is 4096 LDS
  // bytes on = a whole number of 16-row groups further down, so its
  // swizzle and column are the same
  static constexpr int RM_STEP = NTH_KV * 16 / (D * 2);   // rows
  static constexpr int T_STEP = NTH_KV * 16 / 64;         // d rows
  static_assert(RM_STEP % 16 == 0 && T_STEP % 16 == 0, "swizzle period");
  int row_rm, col_rm, off_t;

  DEVINL void init(int S_pad) {
    const int o = threadIdx.x * 16;
    int r, bb;
    unswz(o, D * 2, r, bb);
    row_rm = r;
    col_rm = bb >> 1;
    unswz(o, 64, r, bb);
    off_t = r * S_pad + (bb >> 1);
  }

  // pointers at the (b, hq) head; rcp = the head's [2][S_pad] start
  // values (attn_bwd_pre_kernel); st = destination stage buffer. The
  // transposed planes and rcp are padded to S_pad >= m0 + 32.
  DEVINL void issue(const bf16_t* qp, const bf16_t* dop, const bf16_t* qtp,
                    const bf16_t* dotp, const float* rcp, int m0, int S,
                    long q_tok, int S_pad, char* st) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      char* dst = st + (i * NTH_KV + (threadIdx.x & ~63)) * 16;
      const long go =
          (long)min(m0 + row_rm + i * RM_STEP, S - 1) * q_tok + col_rm;
      const long to = (long)off_t + (long)i * T_STEP * S_pad + m0;
      glds<16>(qp + go, dst);
      glds<16>(dop + go, dst + TB);
      glds<16>(qtp + to, dst + 2 * TB);
      glds<16>(dotp + to, dst + 3 * TB);
    }
    if (threadIdx.x < 64)   // wave 0: 32 S' starts, then 32 dP' starts
      glds<4>(rcp + (threadIdx.x >> 5) * S_pad + m0 + (threadIdx.x & 31),
              st + RC_OFF);
  }

  // retire this wave's DMAs; the caller's barrier makes the stage
  // readable
  DEVINL void finish() const {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
};

// One 32-row q tile against the wave's first NH live 32-key halves, in
// two parts so the caller can turn the prefetch registers over between
// them. Part 1: S' = Q·K^T - lse*sqrt(D) and dP' = dO·V^T - Dsum.
template <int D, int NH>
DEVINL void dkdv_tile_sdp(const char* st, const char* v_lds,
                          const bf16x8v (&k_reg)[2][D / 16],
                          f32x16 (&sv)[2], f32x16 (&dpv)[2], int vrow0,
                          int lane, int hi) {
  constexpr int QC = D / 16;
  constexpr int TB = DkdvStage<D>::TB;
  const char* q_lds = st;
  const char* do_lds = st + TB;
  const char* rc_lds = st + DkdvStage<D>::RC_OFF;

#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4 s4 = *(const f32x4*)(rc_lds + (8 * g + 4 * hi) * 4);
    const f32x4 d4 = *(const f32x4*)(rc_lds + 128 + (8 * g + 4 * hi) * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int hh = 0; hh < NH; ++hh) {
        sv[hh][4 * g + j] = s4[j];
        dpv[hh][4 * g + j] = d4[j];
      }
  }
#pragma unroll
  for (int c = 0; c < QC; ++c) {
    const bf16x8v qa =
        read_bfrag<D * 2>(q_lds, lane & 31, c * 16 + hi * 8);
    const bf16x8v doa =
        read_bfrag<D * 2>(do_lds, lane & 31, c * 16 + hi * 8);
#pragma unroll
    for (int hh = 0; hh < NH; ++hh) {
      sv[hh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          qa, k_reg[hh][c], sv[hh], 0, 0, 0);
      const bf16x8v vb = read_bfrag<D * 2>(
          v_lds, vrow0 + hh * 32 + (lane & 31), c * 16 + hi * 8);
      dpv[hh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          doa, vb, dpv[hh], 0, 0, 0);
    }
  }
}

// Part 2: P = exp2(c2*S'), dS = P*dP', dV += P^T·dO, dK += dS^T·Q.
// Document bounds (DOC): a lane owns one key, so its bound is doc_end of
// that key, one value per 32-key half: q row qg sees the key iff
// kvrow <= qg < dend, which is one unsigned compare, qg - kvrow < dlen,
// with dlen = dend - kvrow (0 for a key past S): as many operations per
// element as the plain chain. The chain is a select under a uniform flag,
// not a branch, so it runs on every tile; with separate compares for the
// causal cut and the bound the whole backward was 6 % slower at one
// document per row (profiles/attn_docs.log). dend_min is the half's
// smallest doc_end (its first key's); the per-element mask is also needed
// once the tile's last real q row reaches it.
template <int D, bool CAUSAL, int NH, bool DOC>
DEVINL void dkdv_tile_acc(const char* st, const f32x16 (&sv)[2],
                          const f32x16 (&dpv)[2],
                          f32x16 (&dk_acc)[2][D / 32],
                          f32x16 (&dv_acc)[2][D / 32], int m0, int n0w,
                          int S, int lane, int hi, float c2,
                          const int (&dlen)[2], const int (&dend_min)[2]) {
  constexpr int DT = D / 32;
  constexpr int TB = DkdvStage<D>::TB;
  const char* qt_lds = st + 2 * TB;
  const char* dot_lds = st + 3 * TB;

  bf16x8v pa[NH][2], da[NH][2];
#pragma unroll
  for (int hh = 0; hh < NH; ++hh) {
    const int ks0 = n0w + hh * 32;
    const int kvrow = ks0 + (lane & 31);
    // q-side padding is already in the row constant; only the diagonal
    // and the key tail need the per-element mask (uniform flag)
    const bool need_mask = (CAUSAL && m0 < ks0 + 32) || (ks0 + 32 > S) ||
                           (DOC && min(m0 + QROWS, S) > dend_min[hh]);
    f32x16 pt, dst;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float pv = __builtin_amdgcn_exp2f(sv[hh][r] * c2);
      if (need_mask) {
        const int qg = m0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (DOC ? !((unsigned)(qg - kvrow) < (unsigned)dlen[hh])
                : !(kvrow < S && (!CAUSAL || qg >= kvrow)))
          pv = 0.f;
      }
      pt[r] = pv;
      dst[r] = pv * dpv[hh][r];
    }
    repack_pa(pt, pa[hh][0], pa[hh][1]);
    repack_pa(dst, da[hh][0], da[hh][1]);
  }

#pragma unroll
  for (int t = 0; t < DT; ++t) {
    const bf16x8v o0 = read_bfrag<64>(dot_lds, t * 32 + (lane & 31), hi * 8);
    const bf16x8v q0 = read_bfrag<64>(qt_lds, t * 32 + (lane & 31), hi * 8);
    const bf16x8v o1 =
        read_bfrag<64>(dot_lds, t * 32 + (lane & 31), 16 + hi * 8);
    const bf16x8v q1 =
        read_bfrag<64>(qt_lds, t * 32 + (lane & 31), 16 + hi * 8);
#pragma unroll
    for (int hh = 0; hh < NH; ++hh) {
      dv_acc[hh][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          pa[hh][0], o0, dv_acc[hh][t], 0, 0, 0);
      dk_acc[hh][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          da[hh][0], q0, dk_acc[hh][t], 0, 0, 0);
    }
#pragma unroll
    for (int hh = 0; hh < NH; ++hh) {
      dv_acc[hh][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          pa[hh][1], o1, dv_acc[hh][t], 0, 0, 0);
      dk_acc[hh][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          da[hh][1], q1, dk_acc[hh][t], 0, 0, 0);
    }
  }
}

template <int D, bool CAUSAL, bool DOC = false, typename... DOCARG>
__global__ __launch_bounds__(NTH_KV) void attn_bwd_dkdv_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ v, const bf16_t* __restrict__ dout,
    const bf16_t* __restrict__ q_t, const bf16_t* __restrict__ dot_t,
    const float* __restrict__ rc, bf16_t* __restrict__ dk,
    bf16_t* __restrict__ dv, int B, int S, int Hq, int Hkv, int S_pad,
    float scale, DOCARG... doc_end) {
  static_assert(sizeof...(DOCARG) == (DOC ? 1 : 0), "one tensor with DOC");
  static_assert(!DOC || CAUSAL, "document bounds refine the causal mask");
  constexpr int QC = D / 16;
  constexpr int DT = D / 32;
  constexpr int BNK = NW_KV * 64;   // 256 keys per block
  constexpr int STB = DkdvStage<D>::BYTES;
  __shared__ __attribute__((aligned(16))) char smem[2 * STB + BNK * D * 2];
  char* v_lds = smem + 2 * STB;

  const int lane = threadIdx.x & 63;
  const int hi = lane >> 5;
  const int wid = threadIdx.x >> 6;
  int bx, hkv, b;
  xcd_block_index(bx, hkv, b);
  const int n0 = bx * BNK;
  const int n0w = n0 + wid * 64;
  const int rep = Hq / Hkv;

  const long q_tok = (long)Hq * D, kv_tok = (long)Hkv * D;
  const bf16_t* kp = k + ((long)b * S * kv_tok) + (long)hkv * D;
  const bf16_t* vp = v + ((long)b * S * kv_tok) + (long)hkv * D;

  bf16x8v k_reg[2][QC];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    const int kvrow = n0w + hh * 32 + (lane & 31);
#pragma unroll
    for (int c = 0; c < QC; ++c) {
      uint4 kr = {0, 0, 0, 0};
      if (kvrow < S)
        kr = *(const uint4*)(kp + (long)kvrow * kv_tok + c * 16 + hi * 8);
      k_reg[hh][c] = as_frag(kr);
    }
  }
  {  // stage the block's 256-row V tile (row-major, swizzled) once
    constexpr int VPR = D / 8;
#pragma unroll 4
    for (int vi = threadIdx.x; vi < BNK * VPR; vi += NTH_KV) {
      const int row = vi / VPR, cv = vi % VPR;
      uint4 val = {0, 0, 0, 0};
      if (n0 + row < S)
        val = *(const uint4*)(vp + (long)(n0 + row) * kv_tok + cv * 8);
      *(uint4*)(v_lds + swz_off(row, D * 2, cv * 16)) = val;
    }
  }

  f32x16 dk_acc[2][DT], dv_acc[2][DT];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        dk_acc[hh][t][r] = 0.f;
        dv_acc[hh][t][r] = 0.f;
      }

  const int m_start = CAUSAL ? n0 : 0;   // n0 is a multiple of QROWS
  // Document bounds: doc_end of the lane's key per half, clamped into
  // (key, S] (keys past S take row S-1's and are masked as keys anyway);
  // each half's smallest and largest value (first / last lane, doc_end is
  // non-decreasing) made wave-uniform; and the end of the block's q loop,
  // doc_end of the block's last key clamped into (n0, S]. No q row at or
  // past m_end can see a key of this block. What stays in a register per
  // half is dlen = doc_end - key (see dkdv_tile_acc). Without DOC the
  // bounds are all S and dlen is unused.
  int dlen[2] = {0, 0}, dend_min[2] = {S, S}, dend_max[2] = {S, S};
  int m_end = S;
  if constexpr (DOC) {
    const int* dep = first_arg(doc_end...) + (long)b * S;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int key = n0w + hh * 32 + (lane & 31);
      const int kvrow = min(key, S - 1);
      const int dend = min(S, max(dep[kvrow], kvrow + 1));
      dlen[hh] = key < S ? dend - key : 0;
      dend_min[hh] = __builtin_amdgcn_readfirstlane(dend);
      dend_max[hh] = __builtin_amdgcn_readlane(dend, 31);
    }
    m_end = min(S, max(dep[min(n0 + BNK, S) - 1], n0 + 1));
  }
  const float c2 = LOG2E * scale;
  const long plane = (long)D * S_pad;
  const long head0 = (long)b * Hq + hkv * rep;
  const bf16_t* qh = q + ((long)b * S * q_tok) + (long)(hkv * rep) * D;
  const bf16_t* doh = dout + ((long)b * S * q_tok) + (long)(hkv * rep) * D;

  DkdvStage<D> stg;
  stg.init(S_pad);
  stg.issue(qh, doh, q_t + head0 * plane, dot_t + head0 * plane,
            rc + head0 * 2 * S_pad, m_start, S, q_tok, S_pad, smem);
  stg.finish();
  __syncthreads();
  int cur = 0;

  for (int g = 0; g < rep; ++g) {
    for (int m0 = m_start; m0 < m_end; m0 += QROWS) {
      const char* st = smem + cur * STB;
      char* nst = smem + (cur ^ 1) * STB;
      // next tile: next q rows of this head, else the next head's first
      int gn = g, mn = m0 + QROWS;
      if (mn >= m_end) {
        gn = g + 1;
        mn = m_start;
      }
      const bool more = gn < rep;
      // wave-uniform skip of key halves with no keys or entirely above
      // the diagonal for this q tile; half 1 live implies half 0 live.
      // With document bounds a half is also dead once the q tile starts
      // past the document of its last key; half 1 can then be live with
      // half 0's keys all masked, which the two-half path handles.
      const bool live0 = n0w < S && (!CAUSAL || m0 + QROWS > n0w) &&
                         (!DOC || m0 < dend_max[0]);
      const bool live1 = n0w + 32 < S &&
                         (!CAUSAL || m0 + QROWS > n0w + 32) &&
                         (!DOC || m0 < dend_max[1]);

      // the other buffer was last read before the previous barrier
      if (more)
        stg.issue(qh + (long)gn * D, doh + (long)gn * D,
                  q_t + (head0 + gn) * plane, dot_t + (head0 + gn) * plane,
                  rc + (head0 + gn) * 2 * S_pad, mn, S, q_tok, S_pad, nst);
      f32x16 sv[2], dpv[2];
      if (live1) {
        dkdv_tile_sdp<D, 2>(st, v_lds, k_reg, sv, dpv, wid * 64, lane, hi);
        dkdv_tile_acc<D, CAUSAL, 2, DOC>(st, sv, dpv, dk_acc, dv_acc, m0,
                                         n0w, S, lane, hi, c2, dlen,
                                         dend_min);
      } else if (live0) {
        dkdv_tile_sdp<D, 1>(st, v_lds, k_reg, sv, dpv, wid * 64, lane, hi);
        dkdv_tile_acc<D, CAUSAL, 1, DOC>(st, sv, dpv, dk_acc, dv_acc, m0,
                                         n0w, S, lane, hi, c2, dlen,
                                         dend_min);
      }
      if (more) stg.finish();
      __syncthreads();
      cur ^= 1;
    }
  }

  bf16_t* dkp = dk + ((long)b * S * kv_tok) + (long)hkv * D;
  bf16_t* dvp = dv + ((long)b * S * kv_tok) + (long)hkv * D;
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = n0w + hh * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
      if (row >= S) continue;
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        const long off = (long)row * kv_tok + t * 32 + (lane & 31);
        dkp[off] = f2bf(dk_acc[hh][t][r] * scale);
        dvp[off] = f2bf(dv_acc[hh][t][r]);
      }
    }
}

// ========================================================================
// Backward dQ v3: grid (ceil(S/256), Hq, B); 8 waves, wave = 32 q rows.
// Q/dO in registers (lane owns q row); lse/Dsum are per-lane scalars.
// ========================================================================
template <int D, bool CAUSAL, bool XCD, bool DOC = false,
          typename... DOCARG>
__global__ __launch_bounds__(NTHREADS) void attn_bwd_dq_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ v, const bf16_t* __restrict__ dout,
    const bf16_t* __restrict__ k_t, const float* __restrict__ lse,
    const float* __restrict__ dsum, bf16_t* __restrict__ dq, int B, int S,
    int Hq, int Hkv, int S_pad, float scale, DOCARG... doc_start) {
  static_assert(sizeof...(DOCARG) == (DOC ? 1 : 0), "one tensor with DOC");
  static_assert(!DOC || CAUSAL, "document bounds refine the causal mask");
  constexpr int QC = D / 16;
  constexpr int DT = D / 32;
  constexpr int BM3 = NW * 32;
  constexpr int KB = BN * D * 2;
  // double-buffered (K rm | KT | V rm): one barrier per kv tile
  __shared__ __attribute__((aligned(16))) char smem[2 * (3 * KB)];

  const int lane = threadIdx.x & 63;
  const int hi = lane >> 5;
  const int wid = threadIdx.x >> 6;
  // causal: the last q block has the most kv tiles; dispatch it first so
  // the grid does not end on a tail of 16-tile blocks (measured -3 % on
  // the whole backward, docs/ROADMAP.md)
  int bx = blockIdx.x, hq = blockIdx.y, b = blockIdx.z;
  if (XCD) xcd_block_index(bx, hq, b);
  const int m0 = (CAUSAL ? (int)(gridDim.x - 1 - bx) : bx) * BM3;
  const int m0w = m0 + wid * 32;
  const int hkv = hq / (Hq / Hkv);

  const long q_tok = (long)Hq * D, kv_tok = (long)Hkv * D;
  const bf16_t* qp = q + ((long)b * S * q_tok) + (long)hq * D;
  const bf16_t* kp = k + ((long)b * S * kv_tok) + (long)hkv * D;
  const bf16_t* vp = v + ((long)b * S * kv_tok) + (long)hkv * D;
  const bf16_t* dop = dout + ((long)b * S * q_tok) + (long)hq * D;
  const bf16_t* ktp = k_t + ((long)b * Hkv + hkv) * (long)D * S_pad;
  const float* lsep = lse + ((long)b * Hq + hq) * S;
  const float* dsp = dsum + ((long)b * Hq + hq) * S;
  bf16_t* dqp = dq + ((long)b * S * q_tok) + (long)hq * D;

  const int qrow = m0w + (lane & 31);
  bf16x8v q_reg[QC], do_reg[QC];
#pragma unroll
  for (int c = 0; c < QC; ++c) {
    uint4 qr = {0, 0, 0, 0}, dor = {0, 0, 0, 0};
    if (qrow < S) {
      qr = *(const uint4*)(qp + (long)qrow * q_tok + c * 16 + hi * 8);
      dor = *(const uint4*)(dop + (long)qrow * q_tok + c * 16 + hi * 8);
    }
    q_reg[c] = as_frag(qr);
    do_reg[c] = as_frag(dor);
  }
  const float lse_lane = (qrow < S) ? lsep[qrow] : NEG_INF;
  const float ds_lane = (qrow < S) ? dsp[qrow] : 0.f;
  // p = exp(s*scale - lse) as exp2(fma(s, c2, nl2)): one fma + one v_exp
  // per score. lse == -inf gives nl2 = +inf; those rows are masked below.
  const float c2 = scale * LOG2E;
  const float nl2 = -lse_lane * LOG2E;

  f32x16 dq_acc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq_acc[t][r] = 0.f;

  const DocRows<DOC> doc(b, S, m0, qrow, doc_start...);
  // With bounds the whole mask chain of a row is one unsigned compare:
  // dstart <= kvg <= qrow, i.e. kvg - dstart < doc_len, with doc_len = 0
  // for a row past S or without an lse (kvg <= qrow < S covers kvg < S).
  // It holds two registers across the key loop where the plain chain holds
  // qrow and lse_lane; a third (the bound next to those two) spilled this
  // kernel at D = 128.
  int doc_len = 0;
  if (DOC)
    doc_len = (qrow < S && lse_lane != NEG_INF) ? qrow - doc.dstart + 1 : 0;

  TileStage<D> k_st, v_st;
  TileStageT<D> kt_st;
  const int n_end = CAUSAL ? min(S, m0 + BM3) : S;
  k_st.issue(kp, doc.n_begin, S, kv_tok);
  v_st.issue(vp, doc.n_begin, S, kv_tok);
  kt_st.issue(ktp, doc.n_begin, S_pad);
  k_st.write_rm(smem);
  kt_st.write(smem + KB);
  v_st.write_rm(smem + 2 * KB);
  __syncthreads();
  int cur = 0;

  for (int n0 = doc.n_begin; n0 < n_end; n0 += BN) {
    char* k_lds = smem + cur * (3 * KB);
    char* kt_lds = k_lds + KB;
    char* v_lds = k_lds + 2 * KB;
    const bool more = n0 + BN < n_end;
    if (more) {
      k_st.issue(kp, n0 + BN, S, kv_tok);
      v_st.issue(vp, n0 + BN, S, kv_tok);
      kt_st.issue(ktp, n0 + BN, S_pad);
    }

    const bool strip_live = (!CAUSAL || (n0 <= m0w + 31)) &&
                            (!DOC || n0 + BN > doc.wave_min);
    if (strip_live) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {   // two 32-kv subtiles
        f32x16 sv, dpv;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          sv[r] = 0.f;
          dpv[r] = 0.f;
        }
#pragma unroll
        for (int c = 0; c < QC; ++c) {
          bf16x8v ka = read_bfrag<D * 2>(
              k_lds, ks * 32 + (lane & 31), c * 16 + hi * 8);
          sv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              ka, q_reg[c], sv, 0, 0, 0);
          bf16x8v va = read_bfrag<D * 2>(
              v_lds, ks * 32 + (lane & 31), c * 16 + hi * 8);
          dpv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              va, do_reg[c], dpv, 0, 0, 0);
        }

        f32x16 dst;
        // interior subtile: every (q, kv) pair of this wave is strictly
        // causal-valid and in-bounds -> the per-element mask chain is
        // dead VALU work (PMC r2: bwd is ~11 VALU/MFMA). One loop with
        // a uniform flag keeps the register footprint shared.
        // Document bounds: a subtile that begins before the wave's largest
        // bound holds keys of an earlier document for some row. Their
        // exp2(s - lse) can be anything up to +inf (lse belongs to another
        // document); it is replaced by 0 before it meets a product.
        const bool need_mask = (CAUSAL && n0 + ks * 32 + 32 > m0w) ||
                               (n0 + ks * 32 + 32 > S) || (m0w + 32 > S) ||
                               (DOC && n0 + ks * 32 < doc.wave_max);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(sv[r], c2, nl2));
          if (need_mask) {
            const int kvg = n0 + ks * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (DOC ? !((unsigned)(kvg - doc.dstart) < (unsigned)doc_len)
                    : !(qrow < S && kvg < S && (!CAUSAL || kvg <= qrow) &&
                        lse_lane != NEG_INF))
              pv = 0.f;
          }
          dst[r] = pv * (dpv[r] - ds_lane);
        }

        bf16x8v da0, da1;
        repack_pa(dst, da0, da1);
#pragma unroll
        for (int t = 0; t < DT; ++t) {
          bf16x8v b0 = read_bfrag<128>(
              kt_lds, t * 32 + (lane & 31), ks * 32 + hi * 8);
          dq_acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              da0, b0, dq_acc[t], 0, 0, 0);
          bf16x8v b1 = read_bfrag<128>(
              kt_lds, t * 32 + (lane & 31), ks * 32 + 16 + hi * 8);
          dq_acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              da1, b1, dq_acc[t], 0, 0, 0);
        }
      }
    }
    if (more) {
      char* nk = smem + (cur ^ 1) * (3 * KB);
      k_st.write_rm(nk);
      kt_st.write(nk + KB);
      v_st.write_rm(nk + 2 * KB);
    }
    __syncthreads();
    cur ^= 1;
  }

#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = m0w + (r & 3) + 8 * (r >> 2) + 4 * hi;
    if (row >= S) continue;
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const int col = t * 32 + (lane & 31);
      dqp[(long)row * q_tok + col] = f2bf(dq_acc[t][r] * scale);
    }
  }
}

// ========================================================================
// Backward dQ v2: grid (ceil(S/256), Hq, B); 4 waves at 1 wave/SIMD, a
// wave owns 64 q rows as two 32-row halves.
//
// Same arithmetic as attn_bwd_dq_kernel (element formula, key order of
// every sum), restructured the way the fused dK+dV kernel was:
//  * Q and dO of both halves stay in registers; every K, V and K^T
//    fragment read from LDS feeds one MFMA per half: half the LDS read
//    traffic per MFMA and two independent accumulator chains in place of
//    the second wave per SIMD.
//  * Reads run ahead of the chains: every fragment is read two chain
//    steps (4-8 MFMAs) before the MFMAs that take it, the second
//    subtile's first ones under the first subtile's last dQ MFMAs
//    (sched_group_barrier), so the waits in front of the MFMAs are
//    counted. Reading whole chains' fragments ahead spilled at D = 128.
//  * The (K | K^T | V) tile is staged one tile ahead by global -> LDS DMA
//    with the swizzle on the source side (see DkdvStage); key rows past S
//    re-read row S-1, their p is 0 through the kvg < S mask, and the K^T
//    plane's pad columns are zero (transpose.hip).
//  * On the diagonal tile the second 32-key subtile lies entirely above
//    the lower half's rows: only the upper half is computed (H0 = 1).
//  * dQ leaves through the block's own LDS as 16-byte row pieces.
// ========================================================================
template <int D>
struct DqStage {
  static constexpr int NV = D / 32;                 // vecs/thread/image
  static constexpr int KB = BN * D * 2;             // bytes per image
  static constexpr int RM_STEP = NTH_KV * 16 / (D * 2);   // key rows
  static constexpr int T_STEP = NTH_KV * 16 / 128;        // d rows
  static_assert(RM_STEP % 16 == 0 && T_STEP % 16 == 0, "swizzle period");
  static_assert(NV * RM_STEP == BN && NV * T_STEP == D, "image coverage");
  int row_rm, col_rm, off_t;

  DEVINL void init(int S_pad) {
    const int o = threadIdx.x * 16;
    int r, bb;
    unswz(o, D * 2, r, bb);
    row_rm = r;
    col_rm = bb >> 1;
    unswz(o, 128, r, bb);
    off_t = r * S_pad + (bb >> 1);
  }

  // pointers at the (b, hkv) head; st = destination buffer (K | K^T | V).
  // n0 + 64 <= S_pad, so the K^T columns are always inside the plane.
  DEVINL void issue(const bf16_t* kp, const bf16_t* vp, const bf16_t* ktp,
                    int n0, int S, long kv_tok, int S_pad, char* st) {
    // the source offsets are recomputed per tile from these three: hoisted
    // out of the tile loop they would hold ~20 registers across it
    int rr = row_rm, cr = col_rm, ot = off_t;
    asm volatile("" : "+v"(rr), "+v"(cr), "+v"(ot));
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      char* dst = st + (i * NTH_KV + (threadIdx.x & ~63)) * 16;
      const long go = (long)min(n0 + rr + i * RM_STEP, S - 1) * kv_tok + cr;
      const long to = (long)ot + (long)i * T_STEP * S_pad + n0;
      glds<16>(kp + go, dst);
      glds<16>(ktp + to, dst + KB);
      glds<16>(vp + go, dst + 2 * KB);
    }
  }

  DEVINL void finish() const {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
};

// Per-lane row constants of one 32-row half (the lane owns row qrow).
struct DqRow {
  int qrow;
  bool ok;        // qrow < S and lse finite
  float nl2, ds;  // -lse*log2(e), Dsum
};

// dS^T of one 32-key subtile for one half, as the dQ product's A-fragments.
template <bool CAUSAL>
DEVINL void dq_ds_frags(const f32x16& sv, const f32x16& dpv, const DqRow& rw,
                        float c2, bool need_mask, int kv0, int S,
                        bf16x8v& da0, bf16x8v& da1) {
  f32x16 dst;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(sv[r], c2, rw.nl2));
    if (need_mask) {
      const int kvg = kv0 + (r & 3) + 8 * (r >> 2);
      if (!(rw.ok && kvg < S && (!CAUSAL || kvg <= rw.qrow))) pv = 0.f;
    }
    dst[r] = pv * (dpv[r] - rw.ds);
  }
  repack_pa(dst, da0, da1);
}

// One 32-key subtile (32 keys from row ks*32 of the tile at k_lds) against
// the halves H0..1. The S and dP chains advance together, one K and one V
// fragment per step feeding 2*NHL MFMAs; the dQ chain takes one K^T
// fragment per step for NHL MFMAs. Every LDS read is issued AH steps
// (S/dP) or 2*AH steps (dQ) ahead of its MFMAs, 4*AH MFMAs with both
// halves live: the last S/dP steps read the first K^T fragments, and with
// FIRST (the tile's first subtile) the last dQ steps read the next
// subtile's first K/V fragments into ka/va. A subtile that is not FIRST
// finds ka/va[0..AH) read on entry.
template <int D, bool CAUSAL, int H0, bool FIRST, int AH>
DEVINL void dq2_subtile(const char* k_lds, int ks,
                        bf16x8v (&ka)[D / 16], bf16x8v (&va)[D / 16],
                        const bf16x8v (&q_reg)[2][D / 16],
                        const bf16x8v (&do_reg)[2][D / 16],
                        f32x16 (&dq_acc)[2][D / 32], const DqRow (&rw)[2],
                        int n0, int m0w, int S, int lane, int hi, float c2) {
  constexpr int QC = D / 16;
  constexpr int DT = D / 32;
  constexpr int NHL = 2 - H0;   // live halves
  constexpr int KB = DqStage<D>::KB;
  constexpr int AHQ = 2 * AH;
  static_assert(2 * DT == QC && AHQ <= QC, "one K^T fragment per dQ step");
  const char* kt_lds = k_lds + KB;
  const char* v_lds = k_lds + 2 * KB;
  const int krow = ks * 32 + (lane & 31);
  auto read_kb = [&](int e) {
    return read_bfrag<128>(kt_lds, (e >> 1) * 32 + (lane & 31),
                           ks * 32 + (e & 1) * 16 + hi * 8);
  };

  f32x16 sv[2], dpv[2];
#pragma unroll
  for (int h = H0; h < 2; ++h)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      sv[h][r] = 0.f;
      dpv[h][r] = 0.f;
    }
  bf16x8v kb[QC];
  __builtin_amdgcn_s_setprio(1);
  if (FIRST) {
#pragma unroll
    for (int c = 0; c < AH; ++c) {
      ka[c] = read_bfrag<D * 2>(k_lds, krow, c * 16 + hi * 8);
      va[c] = read_bfrag<D * 2>(v_lds, krow, c * 16 + hi * 8);
    }
  }
#pragma unroll
  for (int c = 0; c < QC; ++c) {
#pragma unroll
    for (int h = H0; h < 2; ++h) {
      sv[h] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          ka[c], q_reg[h][c], sv[h], 0, 0, 0);
      dpv[h] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          va[c], do_reg[h][c], dpv[h], 0, 0, 0);
    }
    if (c + AH < QC) {
      ka[c + AH] = read_bfrag<D * 2>(k_lds, krow, (c + AH) * 16 + hi * 8);
      va[c + AH] = read_bfrag<D * 2>(v_lds, krow, (c + AH) * 16 + hi * 8);
    } else {
      const int e = 2 * (c + AH - QC);
      kb[e] = read_kb(e);
      kb[e + 1] = read_kb(e + 1);
    }
  }
  if (FIRST) __builtin_amdgcn_sched_group_barrier(0x100, 2 * AH, 0);
#pragma unroll
  for (int c = 0; c < QC; ++c) {
    __builtin_amdgcn_sched_group_barrier(0x008, 2 * NHL, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
  }
  __builtin_amdgcn_s_setprio(0);

  bf16x8v da[2][2];
#pragma unroll
  for (int h = H0; h < 2; ++h) {
    const int m0h = m0w + h * 32;
    const int kvs = n0 + ks * 32;
    const bool need_mask =
        (CAUSAL && kvs + 32 > m0h) || (kvs + 32 > S) || (m0h + 32 > S);
    dq_ds_frags<CAUSAL>(sv[h], dpv[h], rw[h], c2, need_mask, kvs + 4 * hi, S,
                        da[h][0], da[h][1]);
  }

  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int c = 0; c < QC; ++c) {
#pragma unroll
    for (int h = H0; h < 2; ++h)
      dq_acc[h][c >> 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          da[h][c & 1], kb[c], dq_acc[h][c >> 1], 0, 0, 0);
    if (c + AHQ < QC) {
      kb[c + AHQ] = read_kb(c + AHQ);
    } else if (FIRST) {
      const int e = c + AHQ - QC;
      const int e2 = e >> 1;
      if (e & 1)
        va[e2] = read_bfrag<D * 2>(v_lds, krow + 32, e2 * 16 + hi * 8);
      else
        ka[e2] = read_bfrag<D * 2>(k_lds, krow + 32, e2 * 16 + hi * 8);
    }
  }
#pragma unroll
  for (int c = 0; c < (FIRST ? QC : QC - AHQ); ++c) {
    __builtin_amdgcn_sched_group_barrier(0x008, NHL, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
  }
  __builtin_amdgcn_s_setprio(0);
}

template <int D, bool CAUSAL, int AH>
__global__ __launch_bounds__(NTH_KV) void attn_bwd_dq_kernel_v2(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ v, const bf16_t* __restrict__ dout,
    const bf16_t* __restrict__ k_t, const float* __restrict__ lse,
    const float* __restrict__ dsum, bf16_t* __restrict__ dq, int B, int S,
    int Hq, int Hkv, int S_pad, float scale) {
  constexpr int QC = D / 16;
  constexpr int DT = D / 32;
  constexpr int BMQ = NW_KV * 64;   // 256 q rows per block
  constexpr int STB = 3 * DqStage<D>::KB;
  constexpr int OHB = 32 * D * 2;   // a half's dQ rows in the epilogue
  static_assert(NW_KV * 2 * OHB <= 2 * STB, "dQ staging fits the buffers");
  // double-buffered (K rm | KT | V rm): one barrier per kv tile
  __shared__ __attribute__((aligned(16))) char smem[2 * STB];

  const int lane = threadIdx.x & 63;
  const int hi = lane >> 5;
  const int wid = threadIdx.x >> 6;
  // causal: heaviest q block first, as in attn_bwd_dq_kernel
  int bx, hq, b;
  xcd_block_index(bx, hq, b);
  const int m0 = (CAUSAL ? (int)(gridDim.x - 1 - bx) : bx) * BMQ;
  const int m0w = m0 + wid * 64;
  const int hkv = hq / (Hq / Hkv);

  const long q_tok = (long)Hq * D, kv_tok = (long)Hkv * D;
  const bf16_t* qp = q + ((long)b * S * q_tok) + (long)hq * D;
  const bf16_t* kp = k + ((long)b * S * kv_tok) + (long)hkv * D;
  const bf16_t* vp = v + ((long)b * S * kv_tok) + (long)hkv * D;
  const bf16_t* dop = dout + ((long)b * S * q_tok) + (long)hq * D;
  const bf16_t* ktp = k_t + ((long)b * Hkv + hkv) * (long)D * S_pad;
  const float* lsep = lse + ((long)b * Hq + hq) * S;
  const float* dsp = dsum + ((long)b * Hq + hq) * S;
  bf16_t* dqp = dq + ((long)b * S * q_tok) + (long)hq * D;

  const int n_end = CAUSAL ? min(S, m0 + BMQ) : S;
  DqStage<D> stg;
  stg.init(S_pad);
  stg.issue(kp, vp, ktp, 0, S, kv_tok, S_pad, smem);

  bf16x8v q_reg[2][QC], do_reg[2][QC];
  DqRow rw[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int qrow = m0w + h * 32 + (lane & 31);
#pragma unroll
    for (int c = 0; c < QC; ++c) {
      uint4 qr = {0, 0, 0, 0}, dor = {0, 0, 0, 0};
      if (qrow < S) {
        qr = *(const uint4*)(qp + (long)qrow * q_tok + c * 16 + hi * 8);
        dor = *(const uint4*)(dop + (long)qrow * q_tok + c * 16 + hi * 8);
      }
      q_reg[h][c] = as_frag(qr);
      do_reg[h][c] = as_frag(dor);
    }
    const float lse_lane = (qrow < S) ? lsep[qrow] : NEG_INF;
    rw[h].qrow = qrow;
    rw[h].ok = qrow < S && lse_lane != NEG_INF;
    // p = exp(s*scale - lse) as exp2(fma(s, c2, nl2)); lse == -inf gives
    // nl2 = +inf, those rows are masked through ok
    rw[h].nl2 = -lse_lane * LOG2E;
    rw[h].ds = (qrow < S) ? dsp[qrow] : 0.f;
  }
  const float c2 = scale * LOG2E;

  f32x16 dq_acc[2][DT];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) dq_acc[h][t][r] = 0.f;

  stg.finish();
  __syncthreads();
  int cur = 0;

  for (int n0 = 0; n0 < n_end; n0 += BN) {
    const char* k_lds = smem + cur * STB;
    const bool more = n0 + BN < n_end;
    // the other buffer was last read before the previous barrier
    if (more)
      stg.issue(kp, vp, ktp, n0 + BN, S, kv_tok, S_pad,
                smem + (cur ^ 1) * STB);

    // wave-uniform: the wave has rows, and the tile is not entirely above
    // them (m0w and n0 are multiples of 64, so both halves agree)
    const bool live = m0w < S && (!CAUSAL || n0 <= m0w);
    if (live) {
      // the LDS read addresses are cheap functions of the lane; hidden
      // from loop-invariant hoisting they are recomputed per tile, hoisted
      // they take ~40 registers across the loop (spills at D = 128)
      int lane_t = lane;
      asm volatile("" : "+v"(lane_t));
      const int hi_t = lane_t >> 5;
      bf16x8v ka[QC], va[QC];
      dq2_subtile<D, CAUSAL, 0, true, AH>(k_lds, 0, ka, va, q_reg, do_reg,
                                          dq_acc, rw, n0, m0w, S, lane_t,
                                          hi_t, c2);
      // diagonal tile: keys n0+32.. are all above the lower half's rows
      if (CAUSAL && n0 == m0w)
        dq2_subtile<D, CAUSAL, 1, false, AH>(k_lds, 1, ka, va, q_reg, do_reg,
                                             dq_acc, rw, n0, m0w, S, lane_t,
                                             hi_t, c2);
      else
        dq2_subtile<D, CAUSAL, 0, false, AH>(k_lds, 1, ka, va, q_reg, do_reg,
                                             dq_acc, rw, n0, m0w, S, lane_t,
                                             hi_t, c2);
    }
    if (more) stg.finish();
    __syncthreads();
    cur ^= 1;
  }

  // epilogue. Every wave is past the loop's last barrier and no DMA is in
  // flight, so the stage buffers are free and each wave owns 2*OHB bytes.
  // O^T-style fragments -> row-major bf16 rows, then whole 16-byte pieces;
  // the XOR of byte 64 with the row's bit 2 (= hi) keeps the two
  // half-waves' 2-byte writes on disjoint banks (as in the v4 forward).
  constexpr int CPR = D * 2 / 16;   // 16-byte chunks per row
  constexpr int RPI = WAVE / CPR;   // rows per wave-wide store
  // lane-derived epilogue addresses are recomputed here, not carried
  // across the tile loop
  int lane_e = lane;
  asm volatile("" : "+v"(lane_e));
  const int hi_e = lane_e >> 5;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    char* ow = smem + (wid * 2 + h) * OHB;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rowidx = (r & 3) + 8 * (r >> 2) + 4 * hi_e;
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        const int cb = (t * 32 + (lane_e & 31)) * 2;
        *(bf16_t*)(ow + rowidx * (D * 2) + (cb ^ (hi_e << 6))) =
            f2bf(dq_acc[h][t][r] * scale);
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const char* ow = smem + (wid * 2 + h) * OHB;
#pragma unroll
    for (int i = 0; i < 32 / RPI; ++i) {
      const int row = i * RPI + lane_e / CPR;
      const int ch = lane_e % CPR;
      const uint4 val = *(const uint4*)(
          ow + row * (D * 2) + ((ch * 16) ^ (((row >> 2) & 1) << 6)));
      if (m0w + h * 32 + row < S)
        *(uint4*)(dqp + (long)(m0w + h * 32 + row) * q_tok + ch * 8) = val;
    }
  }
}

}  // namespace

extern "C" {

// vt: pre-transposed V plane [B, Hkv, D, S_pad] (tok_transpose_head)
// variant = 0: attn_fwd_kernel_v4 (default); variant = 1: the older v3,
// kept so both can be timed and compared in one process.
hipError_t tok_attn_fwd(const void* q, const void* k, const void* vt, void* o,
                        float* lse, int B, int S, int Hq, int Hkv, int D,
                        int S_pad, int causal, hipStream_t stream,
                        int variant, const int* doc_start) {
  dim3 grid((S + NW * 32 - 1) / (NW * 32), Hq, B);
  const float scale = 1.f / sqrtf((float)D);
  if (variant != 0 && variant != 1) return hipErrorInvalidValue;
  // doc_start: optional int32 [B, S] document bounds (DocRows); only the
  // causal v4 kernel has the instantiation
  if (doc_start) {
    if (!causal || variant != 0) return hipErrorInvalidValue;
    if (D == 128)
      attn_fwd_kernel_v4<128, true, true><<<grid, NTHREADS, 0, stream>>>(
          (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)vt, (bf16_t*)o,
          lse, B, S, Hq, Hkv, S_pad, scale, doc_start);
    else if (D == 64)
      attn_fwd_kernel_v4<64, true, true><<<grid, NTHREADS, 0, stream>>>(
          (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)vt, (bf16_t*)o,
          lse, B, S, Hq, Hkv, S_pad, scale, doc_start);
    else
      return hipErrorInvalidValue;
    return hipGetLastError();
  }
#define LAUNCH_FWD(DD, CC)                                                    \
  do {                                                                        \
    if (variant == 1)                                                         \
      attn_fwd_kernel_v3<DD, CC><<<grid, NTHREADS, 0, stream>>>(              \
          (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)vt, (bf16_t*)o, \
          lse, B, S, Hq, Hkv, S_pad, scale);                                  \
    else                                                                      \
      attn_fwd_kernel_v4<DD, CC><<<grid, NTHREADS, 0, stream>>>(              \
          (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)vt, (bf16_t*)o, \
          lse, B, S, Hq, Hkv, S_pad, scale);                         \
  } while (0)
  if (D == 128) { if (causal) LAUNCH_FWD(128, true); else LAUNCH_FWD(128, false); }
  else if (D == 64) { if (causal) LAUNCH_FWD(64, true); else LAUNCH_FWD(64, false); }
  else return hipErrorInvalidValue;
#undef LAUNCH_FWD
  return hipGetLastError();
}

// q_t/k_t/dot_t: pre-transposed [.., D, S_pad] planes (tok_transpose_head)
// split = 0: pre -> fused dK+dV -> dQ (default); split = 1: pre -> dV ->
// dK -> dQ with the 8-wave split kernels, kept so both paths can be timed
// and compared in one process. dq_variant selects the dQ kernel the same
// way: 1 = the 8-wave attn_bwd_dq_kernel in XCD-aware block order (the
// default of the Python binding), 0 = the 4-wave attn_bwd_dq_kernel_v2
// (same order; measured slower, see there), 2 = the 8-wave kernel in plain
// block order, as it ran before the reordering.
hipError_t tok_attn_bwd(const void* q, const void* k, const void* v,
                        const void* o, const void* dout, const void* q_t,
                        const void* k_t, const void* dot_t, const float* lse,
                        float* dsum_ws, float* rc_ws, void* dq, void* dk,
                        void* dv, int B, int S, int Hq, int Hkv, int D,
                        int S_pad, int causal, hipStream_t stream, int split,
                        int dq_variant, const int* doc_start,
                        const int* doc_end) {
  const float scale = 1.f / sqrtf((float)D);
  if (dq_variant < 0 || dq_variant > 2) return hipErrorInvalidValue;
  // doc_start / doc_end: optional int32 [B, S] document bounds, both or
  // neither; only the causal default pair (fused dK+dV, dq_variant 1) has
  // the instantiations
  const bool docs = doc_start != nullptr;
  if (docs != (doc_end != nullptr)) return hipErrorInvalidValue;
  if (docs && (!causal || split || dq_variant != 1))
    return hipErrorInvalidValue;
  dim3 gpre((S + PRE_ROWS - 1) / PRE_ROWS, Hq, B);
  if (D == 128)
    attn_bwd_pre_kernel<128><<<gpre, 256, 0, stream>>>(
        (const bf16_t*)dout, (const bf16_t*)o, lse, dsum_ws, rc_ws, Hq, S,
        S_pad, 1.f / scale);
  else if (D == 64)
    attn_bwd_pre_kernel<64><<<gpre, 256, 0, stream>>>(
        (const bf16_t*)dout, (const bf16_t*)o, lse, dsum_ws, rc_ws, Hq, S,
        S_pad, 1.f / scale);
  else
    return hipErrorInvalidValue;

  dim3 gkv((S + NW * 32 - 1) / (NW * 32), Hkv, B);
  dim3 gkvf((S + NW_KV * 64 - 1) / (NW_KV * 64), Hkv, B);
  dim3 gq((S + NW * 32 - 1) / (NW * 32), Hq, B);
#define LAUNCH_BWD_DOC(DD)                                                    \
  do {                                                                        \
    attn_bwd_dkdv_kernel<DD, true, true><<<gkvf, NTH_KV, 0, stream>>>(        \
        (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v,                 \
        (const bf16_t*)dout, (const bf16_t*)q_t, (const bf16_t*)dot_t,        \
        rc_ws, (bf16_t*)dk, (bf16_t*)dv, B, S, Hq, Hkv, S_pad, scale,         \
        doc_end);                                                             \
    attn_bwd_dq_kernel<DD, true, true, true><<<gq, NTHREADS, 0, stream>>>(    \
        (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v,                 \
        (const bf16_t*)dout, (const bf16_t*)k_t, lse, dsum_ws,                \
        (bf16_t*)dq, B, S, Hq, Hkv, S_pad, scale,                            \
        doc_start);                                                           \
  } while (0)
  if (docs) {
    if (D == 128) LAUNCH_BWD_DOC(128); else LAUNCH_BWD_DOC(64);
    return hipGetLastError();
  }
#undef LAUNCH_BWD_DOC
#define LAUNCH_BWD(DD, CC)                                                    \
  do {                                                                        \
    if (split) {                                                              \
      attn_bwd_dv_kernel<DD, CC><<<gkv, NTHREADS, 0, stream>>>(               \
          (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)dot_t,           \
          (const bf16_t*)dout, lse, dsum_ws, (bf16_t*)dv, B, S, Hq, Hkv,     \
          S_pad, scale);                                                      \
      attn_bwd_dk_kernel<DD, CC><<<gkv, NTHREADS, 0, stream>>>(               \
          (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v,               \
          (const bf16_t*)dout, (const bf16_t*)q_t, lse, dsum_ws,              \
          (bf16_t*)dk, B, S, Hq, Hkv, S_pad, scale);                          \
    } else {                                                                  \
      attn_bwd_dkdv_kernel<DD, CC><<<gkvf, NTH_KV, 0, stream>>>(              \
          (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v,               \
          (const bf16_t*)dout, (const bf16_t*)q_t, (const bf16_t*)dot_t,      \
          rc_ws, (bf16_t*)dk, (bf16_t*)dv, B, S, Hq, Hkv, S_pad, scale);      \
    }                                                                         \
    if (dq_variant == 0)                                                      \
      attn_bwd_dq_kernel_v2<DD, CC, (CC ? 2 : 1)>                             \
          <<<gq, NTH_KV, 0, stream>>>(                                        \
          (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v,               \
          (const bf16_t*)dout, (const bf16_t*)k_t, lse, dsum_ws,              \
          (bf16_t*)dq, B, S, Hq, Hkv, S_pad, scale);                          \
    else if (dq_variant == 1)                                                 \
      attn_bwd_dq_kernel<DD, CC, true><<<gq, NTHREADS, 0, stream>>>(          \
          (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v,               \
          (const bf16_t*)dout, (const bf16_t*)k_t, lse, dsum_ws,              \
          (bf16_t*)dq, B, S, Hq, Hkv, S_pad, scale);                 \
    else                                                                      \
      attn_bwd_dq_kernel<DD, CC, false><<<gq, NTHREADS, 0, stream>>>(         \
          (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v,               \
          (const bf16_t*)dout, (const bf16_t*)k_t, lse, dsum_ws,              \
          (bf16_t*)dq, B, S, Hq, Hkv, S_pad, scale);                 \
  } while (0)
  if (D == 128) { if (causal) LAUNCH_BWD(128, true); else LAUNCH_BWD(128, false); }
  else { if (causal) LAUNCH_BWD(64, true); else LAUNCH_BWD(64, false); }
#undef LAUNCH_BWD
  return hipGetLastError();
}
}
