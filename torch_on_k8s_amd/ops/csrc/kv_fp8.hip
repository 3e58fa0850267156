// FP8 (OCP e4m3) KV cache for ragged decode on MI355X (gfx950): the decode
// kernel that reads it, the two kernels that write it, and the paged forms
// of those two.
//
// Format. kcache/vcache [B,Tmax,Hkv,D] e4m3 codes (max 448, no infinities,
// 0x7F / 0xFF are NaN), kscale/vscale [B,Tmax,Hkv] fp32; a stored element
// means float(code) * scale[b,t,h]. The quantizer is a function of the bf16
// head row x the bf16 kernels would have stored: amax = max|x|; amax == 0
// gives scale 0 and codes 0; otherwise scale = amax / 448 (fp32) and each
// code is v_cvt_pk_fp8_f32 (round to nearest even) of x * (1 / scale) clamped
// to +-448 in fp32, so that a rounding of the scale never makes a NaN code.
//
//   attn_decode_ragged_fp8_kernel<D, R>  grid (Hkv, B, num_splits), 256 threads
//     The contract of attn_decode_ragged_kernel (decode_ragged.hip): block
//     (hkv, b, z) owns keys [z*chunk, (z+1)*chunk) clipped to
//     clamp(lens[b], 0, Tmax) of one kv head and produces all R query heads
//     from one read of each row; an empty chunk writes m = -inf, l = 0 (or a
//     zero bf16 row) and reads nothing; no atomics, fixed order everywhere.
//     Lane map. A row is LPR = D/8 lanes of 8 BYTES (one 8-byte load, 8
//     codes), so lane c of a row owns elements 8c..8c+7, the q and o state
//     per lane is that of the bf16 kernel, and a wave load covers G = 64/LPR
//     rows: lane = g*LPR + c, wave w, row t = base + u*4G + w*G + g.
//     U = 8 row pairs (8 K + 8 V loads of 8 bytes, and their 8 + 8 scales,
//     each one 4-byte load that the LPR lanes of a row share) are issued per
//     lane before the first is consumed: 128 bytes of rows in flight per lane,
//     as the bf16 kernel's 4 pairs of 16 bytes (U = 4 at R = 8, see
//     f8_rows_in_flight). They are consumed in batches of 4 keys, so the
//     scores alive at once stay s[4][R].
//     Codes become fp32 by v_cvt_pk_f32_fp8, two per instruction: 4 per row
//     instead of the 8 shifts/masks of a bf16 row. The row scales never
//     touch an element: kscale[t] * softmax_scale multiplies the reduced
//     score once per key, vscale[t] multiplies p once per (key, head).
//     A row past the chunk's end is replaced by the chunk's first row (codes
//     AND scales; valid, finite) and its weight forced to 0 by select, so a
//     NaN code or NaN scale beyond lens[b] never reaches a product.
//     Score reduction over the LPR lanes of a row: v_add_f32 with DPP row
//     operations (quad_perm 1,0,3,2; quad_perm 2,3,0,1; row_half_mirror;
//     row_mirror at LPR = 16) instead of the bf16 kernel's __shfl_xor
//     butterfly (one ds_bpermute per step): the same depth, every lane of
//     the row ends with the same sum, no LDS traffic. Timed against the
//     shuffle form in one process: 5-16 % faster at every shape
//     (profiles/decode_fp8.log), so the shuffle form is gone.
//     Online softmax, the in-wave butterfly over lane groups, the fold over
//     waves through LDS and the epilogue are those of the bf16 kernel; with
//     num_splits > 1 the fp32 (m, l, o[D]) partials go to the same workspace
//     layout and tok_attn_ragged_combine folds them.
//     fp32 budget (tests/test_kv_fp8_gpu.py counts k from this): the chains
//     of the bf16 kernel, i.e. n = ceil(min(chunk, T) / (4G)) keys per lane
//     group at 3 roundings each, 2 per merge level (log2 G + 4 waves +
//     splits), the divide; a score is 8 fma + log2 LPR adds + 2 roundings
//     (kscale * softmax_scale, then the product); p * vscale is one more
//     rounding per term of o.
//
//   kv_quantize_append_kernel   grid-stride, 256 threads
//     k, v [B,Tq,Hkv,D] bf16 (k already roped), pos, qlens [B] int32 on the
//     device. Work item = 8 elements (one 16-byte load, one 8-byte store) of
//     one head row of k or v; the D/8 consecutive lanes of a row reduce amax
//     by shuffle; lane 0 of the row stores the scale. Token i of sequence b
//     goes to row pos[b] + i; live iff i < qlens[b] and 0 <= pos[b] + i <
//     Tmax; a dead token writes neither codes nor scale.
//
//   qkv_rope_append_fp8_kernel  grid-stride, 256 threads
//     qkv [B,Tq,(Hq+2Hkv)*D]. Work item = one 8-wide vec of the first half of
//     a head row and its partner in the second half, as
//     qkv_rope_append_chunk_kernel and with its arithmetic per element (fp32,
//     two products and an add, rounded to bf16): q rows are written as bf16
//     (zero for a dead token); a k row is rotated, rounded to bf16, and that
//     bf16 row is quantized; a v row is quantized as it is. amax over the
//     D/16 consecutive lanes of a row by shuffle.
//
//   qkv_rope_append_paged_fp8_kernel / kv_quantize_append_paged_kernel
//     The two kernels above for the paged cache of attn_paged_fp8.hip
//     (kpool/vpool [P,Hkv,64,D] codes, kscale/vscale [P,Hkv,64]), with the
//     destination looked up in the table (KtPagedDest, attn_kv_tile.h) as
//     qkv_rope_append_paged_kernel does: the same quantizer per element, so
//     the same codes and scale for the same token. A token is dead if
//     i >= qlens[b], its position is outside [0, 64 NP) or its table entry is
//     outside [0, P); it writes neither codes nor scale and gets a zero q row.
//
// Resources (hipcc -O3 --offload-arch=gfx950,
// -Rpass-analysis=kernel-resource-usage; scratch is 0 B everywhere):
//   kernel                                 VGPR  AGPR  SGPR  LDS B  waves/SIMD
//   attn_decode_ragged_fp8_kernel<128,1>      80     0    40   2080  6
//   attn_decode_ragged_fp8_kernel<128,2>     111     0    40   4160  4
//   attn_decode_ragged_fp8_kernel<128,4>     162     0    39   8320  3
//   attn_decode_ragged_fp8_kernel<128,8>     256     4    46  16640  1
//   attn_decode_ragged_fp8_kernel<64,1>       80     0    40   1056  6
//   attn_decode_ragged_fp8_kernel<64,2>      111     0    40   2112  4
//   attn_decode_ragged_fp8_kernel<64,4>      160     0    39   4224  3
//   attn_decode_ragged_fp8_kernel<64,8>      256     4    46   8448  1
//   kv_quantize_append_kernel<16|8>        28|26     0    56      0  8
//   qkv_rope_append_fp8_kernel<8|4>           61     0    60      0  8
//   qkv_rope_append_paged_fp8_kernel<8|4>     60     0    64      0  8
//   kv_quantize_append_paged_kernel<16|8>  28|26     0    60      0  8
// (R = 8 keeps 4 values in AGPRs, not in scratch, and runs one wave per
// SIMD where the bf16 kernel runs two.)
#include "attn_kv_tile.h"

extern "C" hipError_t tok_attn_ragged_combine(const float* ws, void* out,
                                              int rows, int Hq, int D,
                                              int num_splits,
                                              hipStream_t stream);

namespace {

constexpr int NW_F8 = 4;
constexpr int NTH_F8 = NW_F8 * WAVE;  // 256
// row pairs in flight per lane. R = 8 fills the 256 VGPRs either way; with 4
// pairs only a handful of values live in AGPRs instead of a third of them.
constexpr int f8_rows_in_flight(int R) { return R == 8 ? 4 : 8; }
constexpr int UB_F8 = 4;              // keys per softmax batch
constexpr float F8_MAX = 448.f;

// 8 e4m3 codes -> fp32; byte j of the pair of dwords is element j
DEVINL void f8_unpack8(const uint2 raw, float* f) {
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw.x, false);
  const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw.x, true);
  const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw.y, false);
  const f32x2 d = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw.y, true);
  f[0] = a[0]; f[1] = a[1]; f[2] = b[0]; f[3] = b[1];
  f[4] = c[0]; f[5] = c[1]; f[6] = d[0]; f[7] = d[1];
}

// 8 fp32 -> 8 e4m3 codes of x * inv, clamped to the finite range first
DEVINL uint2 f8_pack8(const float* x, float inv) {
  float y[8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    y[j] = fminf(fmaxf(x[j] * inv, -F8_MAX), F8_MAX);
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], hi, true);
  return make_uint2((uint32_t)lo, (uint32_t)hi);
}

DEVINL void f8_unpack_bf8(const bf16x8 v, float* f) {
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = bfbits2f(v.h[j]);
}

DEVINL float f8_amax8(const float* f) {
  float a = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) a = fmaxf(a, fabsf(f[j]));
  return a;
}

// max over the N consecutive lanes (N a power of two <= 16) that hold a row
template <int N>
DEVINL float f8_group_max(float a) {
#pragma unroll
  for (int off = N / 2; off > 0; off >>= 1)
    a = fmaxf(a, __shfl_xor(a, off, WAVE));
  return a;
}

template <int CTRL>
DEVINL float f8_dpp(float a) {
  return __int_as_float(__builtin_amdgcn_update_dpp(
      0, __float_as_int(a), CTRL, 0xF, 0xF, false));
}

// sum over the LPR (8 or 16) consecutive lanes of a row; all of them get it
template <int LPR>
DEVINL float f8_row_sum(float a) {
  a += f8_dpp<0xB1>(a);    // quad_perm [1,0,3,2]
  a += f8_dpp<0x4E>(a);    // quad_perm [2,3,0,1]
  a += f8_dpp<0x141>(a);   // row_half_mirror: the other quad of 8
  if constexpr (LPR == 16) a += f8_dpp<0x140>(a);  // row_mirror: other half
  return a;
}

// exp(a - b) for a <= b, with exp(-inf - -inf) = 1
DEVINL float f8_exp_diff(float a, float b) {
  return (a == b) ? 1.f : __expf(a - b);
}

template <int D, int R>
KT_KERNEL __launch_bounds__(NTH_F8) void attn_decode_ragged_fp8_kernel(
    const bf16_t* __restrict__ q, const uint8_t* __restrict__ k,
    const uint8_t* __restrict__ v, const float* __restrict__ kscale,
    const float* __restrict__ vscale, const int* __restrict__ lens,
    bf16_t* __restrict__ out, float* __restrict__ ws, int Tmax, int Hkv,
    int chunk, float scale) {
  constexpr int LPR = D / 8;          // lanes per row, 8 bytes each
  constexpr int G = WAVE / LPR;       // rows per wave load
  constexpr int RPS = NW_F8 * G;      // rows per block step
  constexpr int U_F8 = f8_rows_in_flight(R);
  static_assert(LPR == 8 || LPR == 16, "D is 64 or 128");
  __shared__ __attribute__((aligned(16))) float o_slab[NW_F8][R][D];
  __shared__ float m_slab[NW_F8][R], l_slab[NW_F8][R];

  const int hkv = blockIdx.x, b = blockIdx.y, sp = blockIdx.z;
  const int B = gridDim.y, S = gridDim.z;
  const int Hq = Hkv * R;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int g = lane / LPR, c = lane % LPR;

  const int len = min(max(lens[b], 0), Tmax);
  const int c0 = sp * chunk;
  const int c1 = min(c0 + chunk, len);

  // where thread (fr, fc) of the first R*LPR threads puts its 8 outputs
  const int fr = tid / LPR, fc = tid % LPR;
  const long row_o = (long)b * Hq + hkv * R + fr;         // [B,Hq] index
  float* ws_o = ws + (row_o * S + sp) * D + fc * 8;
  float* ws_ml = ws + (long)B * Hq * S * D + (row_o * S + sp) * 2;

  if (c0 >= c1) {  // block-uniform: nothing of this chunk is valid
    if (tid < R * LPR) {
      if (S == 1) {
        bf16x8 z;
#pragma unroll
        for (int j = 0; j < 8; ++j) z.h[j] = 0;
        *reinterpret_cast<bf16x8*>(out + row_o * D + fc * 8) = z;
      } else {
        f32x4v z = {{0.f, 0.f, 0.f, 0.f}};
        reinterpret_cast<f32x4v*>(ws_o)[0] = z;
        reinterpret_cast<f32x4v*>(ws_o)[1] = z;
        if (fc == 0) {
          ws_ml[0] = -INFINITY;
          ws_ml[1] = 0.f;
        }
      }
    }
    return;
  }

  float qr[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r)
    f8_unpack_bf8(*reinterpret_cast<const bf16x8*>(
                      q + ((long)b * Hq + hkv * R + r) * D + c * 8),
                  qr[r]);

  float m[R], l[R], o[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[r][j] = 0.f;
  }

  const long rs = (long)Hkv * D;  // bytes between two cache rows
  const uint8_t* kb = k + (long)b * Tmax * rs + (long)hkv * D + c * 8;
  const uint8_t* vb = v + (long)b * Tmax * rs + (long)hkv * D + c * 8;
  const float* ksb = kscale + (long)b * Tmax * Hkv + hkv;
  const float* vsb = vscale + (long)b * Tmax * Hkv + hkv;

  for (int base = c0; base < c1; base += U_F8 * RPS) {
    const int t0 = base + wid * G + g;
    uint2 kraw[U_F8], vraw[U_F8];
    float ksc[U_F8], vsc[U_F8];
    // all loads first. A row past the chunk's end is replaced by the
    // chunk's first row (valid, finite) and its weight forced to 0 below.
#pragma unroll
    for (int u = 0; u < U_F8; ++u) {
      const int t = t0 + u * RPS;
      const long tt = (t < c1) ? t : c0;
      kraw[u] = *reinterpret_cast<const uint2*>(kb + tt * rs);
      vraw[u] = *reinterpret_cast<const uint2*>(vb + tt * rs);
      ksc[u] = ksb[tt * Hkv];
      vsc[u] = vsb[tt * Hkv];
    }
#pragma unroll
    for (int h = 0; h < U_F8 / UB_F8; ++h) {
      bool ok[UB_F8];
      float s[UB_F8][R];
#pragma unroll
      for (int u = 0; u < UB_F8; ++u) {
        const int uu = h * UB_F8 + u;
        ok[u] = t0 + uu * RPS < c1;
        float kf[8];
        f8_unpack8(kraw[uu], kf);
        const float kq = ksc[uu] * scale;  // once per key
#pragma unroll
        for (int r = 0; r < R; ++r) {
          float a = 0.f;
#pragma unroll
          for (int j = 0; j < 8; ++j) a = fmaf(qr[r][j], kf[j], a);
          a = f8_row_sum<LPR>(a);
          s[u][r] = ok[u] ? a * kq : -INFINITY;
        }
      }
      float vf[UB_F8][8];
#pragma unroll
      for (int u = 0; u < UB_F8; ++u) f8_unpack8(vraw[h * UB_F8 + u], vf[u]);
      // one rescale of (l, o) per 4 keys
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float mn = m[r];
#pragma unroll
        for (int u = 0; u < UB_F8; ++u) mn = fmaxf(mn, s[u][r]);
        const float alpha = f8_exp_diff(m[r], mn);
        float p[UB_F8], pv[UB_F8];
#pragma unroll
        for (int u = 0; u < UB_F8; ++u) {
          p[u] = ok[u] ? __expf(s[u][r] - mn) : 0.f;
          pv[u] = p[u] * vsc[h * UB_F8 + u];  // once per (key, head)
        }
        m[r] = mn;
        l[r] = fmaf(l[r], alpha, (p[0] + p[1]) + (p[2] + p[3]));
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float acc = o[r][j] * alpha;
#pragma unroll
          for (int u = 0; u < UB_F8; ++u) acc = fmaf(pv[u], vf[u][j], acc);
          o[r][j] = acc;
        }
      }
    }
  }

  // lane groups of a wave: butterfly, every lane ends with the wave's state
#pragma unroll
  for (int off = LPR; off < WAVE; off <<= 1) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float m2 = __shfl_xor(m[r], off, WAVE);
      const float l2 = __shfl_xor(l[r], off, WAVE);
      const float M = fmaxf(m[r], m2);
      const float a1 = f8_exp_diff(m[r], M), a2 = f8_exp_diff(m2, M);
      m[r] = M;
      l[r] = fmaf(l2, a2, l[r] * a1);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o[r][j] = fmaf(__shfl_xor(o[r][j], off, WAVE), a2, o[r][j] * a1);
    }
  }
  if (g == 0) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      f32x4v lo = {{o[r][0], o[r][1], o[r][2], o[r][3]}};
      f32x4v hi = {{o[r][4], o[r][5], o[r][6], o[r][7]}};
      reinterpret_cast<f32x4v*>(&o_slab[wid][r][c * 8])[0] = lo;
      reinterpret_cast<f32x4v*>(&o_slab[wid][r][c * 8])[1] = hi;
      if (c == 0) {
        m_slab[wid][r] = m[r];
        l_slab[wid][r] = l[r];
      }
    }
  }
  __syncthreads();

  // waves, in wave order
  if (tid < R * LPR) {
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < NW_F8; ++w) M = fmaxf(M, m_slab[w][fr]);
    float L = 0.f, acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int w = 0; w < NW_F8; ++w) {
      const float mw = m_slab[w][fr];
      const float sw = (mw == -INFINITY) ? 0.f : __expf(mw - M);
      L = fmaf(l_slab[w][fr], sw, L);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        acc[j] = fmaf(o_slab[w][fr][fc * 8 + j], sw, acc[j]);
    }
    if (S == 1) {
      const float inv = (L > 0.f) ? 1.f / L : 0.f;
      bf16x8 ov;
#pragma unroll
      for (int j = 0; j < 8; ++j) ov.h[j] = f2bfbits(acc[j] * inv);
      *reinterpret_cast<bf16x8*>(out + row_o * D + fc * 8) = ov;
    } else {
      f32x4v lo = {{acc[0], acc[1], acc[2], acc[3]}};
      f32x4v hi = {{acc[4], acc[5], acc[6], acc[7]}};
      reinterpret_cast<f32x4v*>(ws_o)[0] = lo;
      reinterpret_cast<f32x4v*>(ws_o)[1] = hi;
      if (fc == 0) {
        ws_ml[0] = M;
        ws_ml[1] = L;
      }
    }
  }
}

// scale and 1/scale of a row from its amax (0, 0 for an all-zero row)
DEVINL void f8_row_scale(float amax, float* scale, float* inv) {
  const float s = amax / F8_MAX;
  *scale = (amax > 0.f) ? s : 0.f;
  *inv = (amax > 0.f) ? 1.f / s : 0.f;
}

// Work item = 8 elements of one head row of k (which = 0) or v (which = 1).
// Dest (attn_kv_tile.h) says where a token's row goes, or that it is dead.
template <int LPR, class Dest>
DEVINL void f8_quantize_append(
    const bf16x8* __restrict__ k, const bf16x8* __restrict__ v,
    uint2* __restrict__ kcache, uint2* __restrict__ vcache,
    float* __restrict__ kscale, float* __restrict__ vscale,
    const int* __restrict__ pos, const int* __restrict__ qlens,
    const Dest& dest, int B, int Tq, int Hkv) {
  // nwork is a multiple of LPR and LPR divides the block: the lanes of a row
  // enter and leave the loop together
  const long nwork = (long)B * Tq * 2 * Hkv * LPR;
  for (long i = (long)blockIdx.x * KT_NTH + threadIdx.x; i < nwork;
       i += (long)gridDim.x * KT_NTH) {
    const long row = i / LPR;                   // (tok*2 + which)*Hkv + h
    const int c = (int)(i - row * LPR);
    const long tw = row / Hkv;                  // tok*2 + which
    const int h = (int)(row - tw * Hkv);
    const long tok = tw >> 1;                   // b*Tq + t
    const bool isv = tw & 1;
    const int b = (int)(tok / Tq);
    const int t = (int)(tok - (long)b * Tq);
    const long dst = dest.row(b, (long)pos[b] + t, t < qlens[b], h);
    float x[8];
    f8_unpack_bf8((isv ? v : k)[(tok * Hkv + h) * LPR + c], x);
    const float amax = f8_group_max<LPR>(f8_amax8(x));
    float scale, inv;
    f8_row_scale(amax, &scale, &inv);
    uint2 codes = f8_pack8(x, inv);
    if (!(amax > 0.f)) codes = make_uint2(0u, 0u);
    if (dst >= 0) {
      (isv ? vcache : kcache)[dst * LPR + c] = codes;
      if (c == 0) (isv ? vscale : kscale)[dst] = scale;
    }
  }
}

template <int LPR>
KT_KERNEL void kv_quantize_append_kernel(
    const bf16x8* __restrict__ k, const bf16x8* __restrict__ v,
    uint2* __restrict__ kcache, uint2* __restrict__ vcache,
    float* __restrict__ kscale, float* __restrict__ vscale,
    const int* __restrict__ pos, const int* __restrict__ qlens, int B, int Tq,
    int Tmax, int Hkv) {
  f8_quantize_append<LPR>(k, v, kcache, vcache, kscale, vscale, pos, qlens,
                          KtContigDest{Tmax, Hkv}, B, Tq, Hkv);
}

template <int LPR>
KT_KERNEL void kv_quantize_append_paged_kernel(
    const bf16x8* __restrict__ k, const bf16x8* __restrict__ v,
    uint2* __restrict__ kpool, uint2* __restrict__ vpool,
    float* __restrict__ kscale, float* __restrict__ vscale,
    const int* __restrict__ pos, const int* __restrict__ qlens,
    const int* __restrict__ page_table, int B, int Tq, int NP, int P,
    int Hkv) {
  f8_quantize_append<LPR>(k, v, kpool, vpool, kscale, vscale, pos, qlens,
                          KtPagedDest{page_table, NP, P, Hkv}, B, Tq, Hkv);
}

// Work item = one 8-wide vec of the first half of one head row of one token
// and its partner in the second half, as qkv_rope_append_chunk_kernel.
template <int HV /* (D/2)/8 */>
KT_KERNEL void qkv_rope_append_fp8_kernel(
    const bf16x8* __restrict__ qkv, bf16x8* __restrict__ q,
    uint2* __restrict__ kcache, uint2* __restrict__ vcache,
    float* __restrict__ kscale, float* __restrict__ vscale,
    const float* __restrict__ tab_cos, const float* __restrict__ tab_sin,
    const int* __restrict__ pos, const int* __restrict__ qlens, int B, int Tq,
    int Tmax, int Hq, int Hkv) {
  constexpr int hv = HV;
  const int heads_total = Hq + 2 * Hkv;
  constexpr int dv8 = hv * 2;  // vecs per head (D/8)
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
    const bool live = t < qlens[b] && p >= 0 && p < Tmax;
    const bool isq = h < Hq;
    const bool isk = !isq && h < Hq + Hkv;
    // head row, uniform over the hv lanes that hold it
    if (!live) {
      if (isq) {  // zero q row, caches untouched
        bf16x8 z;
#pragma unroll
        for (int j = 0; j < 8; ++j) z.h[j] = 0;
        bf16x8* dst = q + (tok * Hq + h) * dv8;
        dst[c] = z;
        dst[c + hv] = z;
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
      bf16x8* dst = q + (tok * Hq + h) * dv8;
      dst[c] = o1;
      dst[c + hv] = o2;
      continue;
    }
    // the bf16 row the bf16 kernels would have stored, quantized
    float f1[8], f2[8];
    f8_unpack_bf8(o1, f1);
    f8_unpack_bf8(o2, f2);
    const float amax =
        f8_group_max<HV>(fmaxf(f8_amax8(f1), f8_amax8(f2)));
    float scale, inv;
    f8_row_scale(amax, &scale, &inv);
    uint2 c1 = f8_pack8(f1, inv), c2 = f8_pack8(f2, inv);
    if (!(amax > 0.f)) c1 = c2 = make_uint2(0u, 0u);
    const int hh = isk ? h - Hq : h - Hq - Hkv;
    const long dst = ((long)b * Tmax + p) * Hkv + hh;
    uint2* cache = isk ? kcache : vcache;
    cache[dst * dv8 + c] = c1;
    cache[dst * dv8 + c + hv] = c2;
    if (c == 0) (isk ? kscale : vscale)[dst] = scale;
  }
}

// Work item = one 8-wide vec of the first half of one head row of one token
// and its partner in the second half, as qkv_rope_append_fp8_kernel.
template <int HV /* (D/2)/8 */>
KT_KERNEL void qkv_rope_append_paged_fp8_kernel(
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
  for (long i = (long)blockIdx.x * KT_NTH + threadIdx.x; i < nwork;
       i += (long)gridDim.x * KT_NTH) {
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
        KtPagedDest{page_table, NP, P, Hkv}.row(b, p, t < qlens[b], hh);
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
    f8_unpack_bf8(o1, f1);
    f8_unpack_bf8(o2, f2);
    const float amax = f8_group_max<HV>(fmaxf(f8_amax8(f1), f8_amax8(f2)));
    float scale, inv;
    f8_row_scale(amax, &scale, &inv);
    uint2 c1 = f8_pack8(f1, inv), c2 = f8_pack8(f2, inv);
    if (!(amax > 0.f)) c1 = c2 = make_uint2(0u, 0u);
    uint2* pool = isk ? kpool : vpool;
    pool[dst * dv8 + c] = c1;
    pool[dst * dv8 + c + hv] = c2;
    if (c == 0) (isk ? kscale : vscale)[dst] = scale;
  }
}

template <int D, int R>
void launch_fp8(const void* q, const void* k, const void* v,
                const float* kscale, const float* vscale, const int* lens,
                void* out, float* ws, int B, int Tmax, int Hkv,
                int num_splits, int chunk, hipStream_t stream) {
  dim3 grid(Hkv, B, num_splits);
  const float scale = 1.f / sqrtf((float)D);
  attn_decode_ragged_fp8_kernel<D, R><<<grid, NTH_F8, 0, stream>>>(
      (const bf16_t*)q, (const uint8_t*)k, (const uint8_t*)v, kscale, vscale,
      lens, (bf16_t*)out, ws, Tmax, Hkv, chunk, scale);
}

template <int D>
bool launch_fp8_r(int R, const void* q, const void* k, const void* v,
                  const float* kscale, const float* vscale, const int* lens,
                  void* out, float* ws, int B, int Tmax, int Hkv,
                  int num_splits, int chunk, hipStream_t stream) {
#define F8_CASE(r)                                                          \
  case r:                                                                   \
    launch_fp8<D, r>(q, k, v, kscale, vscale, lens, out, ws, B, Tmax, Hkv,  \
                     num_splits, chunk, stream);                            \
    return true;
  switch (R) {
    F8_CASE(1) F8_CASE(2) F8_CASE(4) F8_CASE(8)
    default: return false;
  }
#undef F8_CASE
}

}  // namespace

extern "C" {

// ws: fp32, B*Hq*num_splits*(D+2) elements; unused when num_splits == 1.
hipError_t tok_attn_decode_ragged_fp8(const void* q, const void* k,
                                      const void* v, const float* kscale,
                                      const float* vscale, const int* lens,
                                      void* out, float* ws, int B, int Tmax,
                                      int Hq, int Hkv, int D, int num_splits,
                                      int chunk, hipStream_t stream) {
  if (Hkv < 1 || Hq % Hkv != 0 || num_splits < 1 || chunk < 1 ||
      (long)num_splits * chunk < Tmax)
    return hipErrorInvalidValue;
  const int R = Hq / Hkv;
  bool ok = false;
  if (D == 128)
    ok = launch_fp8_r<128>(R, q, k, v, kscale, vscale, lens, out, ws, B, Tmax,
                           Hkv, num_splits, chunk, stream);
  else if (D == 64)
    ok = launch_fp8_r<64>(R, q, k, v, kscale, vscale, lens, out, ws, B, Tmax,
                          Hkv, num_splits, chunk, stream);
  if (!ok) return hipErrorInvalidValue;
  HIP_CHECK(hipGetLastError());
  if (num_splits > 1)
    HIP_CHECK(tok_attn_ragged_combine(ws, out, B, Hq, D, num_splits, stream));
  return hipSuccess;
}

hipError_t tok_kv_quantize_append(const void* k, const void* v, void* kcache,
                                  void* vcache, float* kscale, float* vscale,
                                  const int* pos, const int* qlens, int B,
                                  int Tq, int Tmax, int Hkv, int D,
                                  hipStream_t stream) {
  const int grid = kt_append_grid((long)B * Tq * 2 * Hkv * (D / 8));
  if (D == 128)
    kv_quantize_append_kernel<16><<<grid, KT_NTH, 0, stream>>>(
        (const bf16x8*)k, (const bf16x8*)v, (uint2*)kcache, (uint2*)vcache,
        kscale, vscale, pos, qlens, B, Tq, Tmax, Hkv);
  else if (D == 64)
    kv_quantize_append_kernel<8><<<grid, KT_NTH, 0, stream>>>(
        (const bf16x8*)k, (const bf16x8*)v, (uint2*)kcache, (uint2*)vcache,
        kscale, vscale, pos, qlens, B, Tq, Tmax, Hkv);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t tok_kv_quantize_append_paged(const void* k, const void* v,
                                        void* kpool, void* vpool,
                                        float* kscale, float* vscale,
                                        const int* pos, const int* qlens,
                                        const int* page_table, int B, int Tq,
                                        int NP, int P, int Hkv, int D,
                                        hipStream_t stream) {
  const int grid = kt_append_grid((long)B * Tq * 2 * Hkv * (D / 8));
  if (D == 128)
    kv_quantize_append_paged_kernel<16><<<grid, KT_NTH, 0, stream>>>(
        (const bf16x8*)k, (const bf16x8*)v, (uint2*)kpool, (uint2*)vpool,
        kscale, vscale, pos, qlens, page_table, B, Tq, NP, P, Hkv);
  else if (D == 64)
    kv_quantize_append_paged_kernel<8><<<grid, KT_NTH, 0, stream>>>(
        (const bf16x8*)k, (const bf16x8*)v, (uint2*)kpool, (uint2*)vpool,
        kscale, vscale, pos, qlens, page_table, B, Tq, NP, P, Hkv);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t tok_qkv_rope_append_fp8(const void* qkv, void* q, void* kcache,
                                   void* vcache, float* kscale, float* vscale,
                                   const float* cos_tab, const float* sin_tab,
                                   const int* pos, const int* qlens, int B,
                                   int Tq, int Tmax, int Hq, int Hkv, int D,
                                   hipStream_t stream) {
  const int grid =
      kt_append_grid((long)B * Tq * (Hq + 2 * Hkv) * ((D / 2) / 8));
  if (D == 128)
    qkv_rope_append_fp8_kernel<8><<<grid, KT_NTH, 0, stream>>>(
        (const bf16x8*)qkv, (bf16x8*)q, (uint2*)kcache, (uint2*)vcache, kscale,
        vscale, cos_tab, sin_tab, pos, qlens, B, Tq, Tmax, Hq, Hkv);
  else if (D == 64)
    qkv_rope_append_fp8_kernel<4><<<grid, KT_NTH, 0, stream>>>(
        (const bf16x8*)qkv, (bf16x8*)q, (uint2*)kcache, (uint2*)vcache, kscale,
        vscale, cos_tab, sin_tab, pos, qlens, B, Tq, Tmax, Hq, Hkv);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t tok_qkv_rope_append_paged_fp8(
    const void* qkv, void* q, void* kpool, void* vpool, float* kscale,
    float* vscale, const float* cos_tab, const float* sin_tab, const int* pos,
    const int* qlens, const int* page_table, int B, int Tq, int NP, int P,
    int Hq, int Hkv, int D, hipStream_t stream) {
  const int grid =
      kt_append_grid((long)B * Tq * (Hq + 2 * Hkv) * ((D / 2) / 8));
  if (D == 128)
    qkv_rope_append_paged_fp8_kernel<8><<<grid, KT_NTH, 0, stream>>>(
        (const bf16x8*)qkv, (bf16x8*)q, (uint2*)kpool, (uint2*)vpool, kscale,
        vscale, cos_tab, sin_tab, pos, qlens, page_table, B, Tq, NP, P, Hq,
        Hkv);
  else if (D == 64)
    qkv_rope_append_paged_fp8_kernel<4><<<grid, KT_NTH, 0, stream>>>(
        (const bf16x8*)qkv, (bf16x8*)q, (uint2*)kpool, (uint2*)vpool, kscale,
        vscale, cos_tab, sin_tab, pos, qlens, page_table, B, Tq, NP, P, Hq,
        Hkv);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}
}
