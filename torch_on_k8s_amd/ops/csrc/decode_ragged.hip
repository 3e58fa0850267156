// Ragged-batch single-token attention decode for MI355X (gfx950), and the
// append of the new token's K/V that goes with it.
//
//   attn_decode_ragged_kernel<D, R>   grid (Hkv, B, num_splits), 256 threads
//     q [B,Hq,D], kcache/vcache [B,Tmax,Hkv,D], lens [B] int32 on the device.
//     Sequence b attends to rows [0, clamp(lens[b], 0, Tmax)). A block owns
//     one kv head of one sequence and the keys [z*chunk, (z+1)*chunk) of it,
//     and produces all R = Hq/Hkv query heads of that kv head from ONE read
//     of each K and V row (the older decode.hip reads each row R times).
//     A row is D/8 lanes of 16 bytes, so a wave load covers G = 64/(D/8)
//     rows; rows go straight to VGPRs, no LDS staging (each is used once).
//     U = 4 row pairs (4 K + 4 V loads) are issued per lane before the first
//     is consumed. The score reduction runs over the D/8 lanes of a row
//     only. Online-softmax state (m, l, o[8]) is kept per (head, lane
//     group); groups merge in-wave by shuffle, waves through LDS in wave
//     order. With num_splits == 1 the block writes bf16 `out` itself;
//     otherwise it writes an fp32 partial (m, l, o[D]) per head and
//   attn_decode_ragged_combine        grid (Hq, B), D threads
//     folds the partials in split order. A chunk at or beyond lens[b]
//     writes m = -inf, l = 0 and reads no q, K or V; lens[b] == 0 gives an
//     exactly-zero row. The grid depends on shapes alone and nothing uses
//     atomics: capturable, and bitwise repeatable.
//
//   qkv_rope_append_kernel            grid-stride, 256 threads
//     qkv [B,(Hq+2Hkv)*D] (one token per sequence), pos [B] int32 on the
//     device: rotates q and k of sequence b at pos[b] (fp32, two products
//     and an add per element, as qkv_rope_kernel) and writes k and the v copy
//     into cache[b, pos[b]]. pos[b] outside [0, Tmax) writes nothing to the
//     caches and gives a zero q row.
//
// Resources (hipcc -O3 --offload-arch=gfx950,
// -Rpass-analysis=kernel-resource-usage; scratch is 0 B everywhere):
//   kernel                              VGPR  SGPR  LDS B  waves/SIMD
//   attn_decode_ragged_kernel<128,1>      74    30   2080  6
//   attn_decode_ragged_kernel<128,2>      98    30   4160  4
//   attn_decode_ragged_kernel<128,4>     164    30   8320  3
//   attn_decode_ragged_kernel<128,8>     251    30  16640  2
//   attn_decode_ragged_kernel<64,1>       76    30   1056  6
//   attn_decode_ragged_kernel<64,2>      102    34   2112  4
//   attn_decode_ragged_kernel<64,4>      153    30   4224  3
//   attn_decode_ragged_kernel<64,8>      252    30   8448  2
//   attn_decode_ragged_combine            12    34      0  8
//   qkv_rope_append_kernel                52    64      0  8
#include "common.h"

namespace {

constexpr int NW_RAG = 4;
constexpr int NTH_RAG = NW_RAG * WAVE;  // 256
constexpr int U_RAG = 4;                // row pairs in flight per lane

DEVINL void unpack8(const bf16x8 v, float* f) {
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = bfbits2f(v.h[j]);
}

// exp(a - b) for a <= b, with exp(-inf - -inf) = 1 (an empty state merged
// into an empty state stays empty instead of turning into NaN)
DEVINL float exp_diff(float a, float b) {
  return (a == b) ? 1.f : __expf(a - b);
}

template <int D, int R>
__global__ __launch_bounds__(NTH_RAG) void attn_decode_ragged_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ v, const int* __restrict__ lens,
    bf16_t* __restrict__ out, float* __restrict__ ws, int Tmax, int Hkv,
    int chunk, float scale) {
  constexpr int LPR = D / 8;          // lanes per row
  constexpr int G = WAVE / LPR;       // rows per wave load
  constexpr int RPS = NW_RAG * G;     // rows per block step
  __shared__ __attribute__((aligned(16))) float o_slab[NW_RAG][R][D];
  __shared__ float m_slab[NW_RAG][R], l_slab[NW_RAG][R];

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
    unpack8(*reinterpret_cast<const bf16x8*>(
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

  const long rs = (long)Hkv * D;  // elements between two cache rows
  const bf16_t* kb = k + (long)b * Tmax * rs + (long)hkv * D + c * 8;
  const bf16_t* vb = v + (long)b * Tmax * rs + (long)hkv * D + c * 8;

  for (int base = c0; base < c1; base += U_RAG * RPS) {
    const int t0 = base + wid * G + g;
    bf16x8 kraw[U_RAG], vraw[U_RAG];
    bool ok[U_RAG];
    // all loads first. A row past the chunk's end is replaced by the
    // chunk's first row (valid, finite) and its weight forced to 0 below.
#pragma unroll
    for (int u = 0; u < U_RAG; ++u) {
      const int t = t0 + u * RPS;
      ok[u] = t < c1;
      const long off = (long)(ok[u] ? t : c0) * rs;
      kraw[u] = *reinterpret_cast<const bf16x8*>(kb + off);
      vraw[u] = *reinterpret_cast<const bf16x8*>(vb + off);
    }
    float s[U_RAG][R];
#pragma unroll
    for (int u = 0; u < U_RAG; ++u) {
      float kf[8];
      unpack8(kraw[u], kf);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) a = fmaf(qr[r][j], kf[j], a);
#pragma unroll
        for (int off = LPR / 2; off > 0; off >>= 1)
          a += __shfl_xor(a, off, WAVE);
        s[u][r] = ok[u] ? a * scale : -INFINITY;
      }
    }
    float vf[U_RAG][8];
#pragma unroll
    for (int u = 0; u < U_RAG; ++u) unpack8(vraw[u], vf[u]);
    // one rescale of (l, o) per U keys
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float mn = m[r];
#pragma unroll
      for (int u = 0; u < U_RAG; ++u) mn = fmaxf(mn, s[u][r]);
      const float alpha = exp_diff(m[r], mn);
      float p[U_RAG];
#pragma unroll
      for (int u = 0; u < U_RAG; ++u)
        p[u] = ok[u] ? __expf(s[u][r] - mn) : 0.f;
      m[r] = mn;
      l[r] = fmaf(l[r], alpha, (p[0] + p[1]) + (p[2] + p[3]));
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float acc = o[r][j] * alpha;
#pragma unroll
        for (int u = 0; u < U_RAG; ++u) acc = fmaf(p[u], vf[u][j], acc);
        o[r][j] = acc;
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
      const float a1 = exp_diff(m[r], M), a2 = exp_diff(m2, M);
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
    for (int w = 0; w < NW_RAG; ++w) M = fmaxf(M, m_slab[w][fr]);
    float L = 0.f, acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int w = 0; w < NW_RAG; ++w) {
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

// grid (Hq, B), D threads: fold the S partials of one output row in split
// order.
__global__ void attn_decode_ragged_combine(const float* __restrict__ ws,
                                           bf16_t* __restrict__ out, int S,
                                           int D) {
  const int h = blockIdx.x, b = blockIdx.y, Hq = gridDim.x, B = gridDim.y;
  const int d = threadIdx.x;
  const long row = (long)b * Hq + h;
  const float* po = ws + row * S * D + d;
  const float* pml = ws + (long)B * Hq * S * D + row * S * 2;
  float M = -INFINITY;
  for (int s = 0; s < S; ++s) M = fmaxf(M, pml[2 * s]);
  float L = 0.f, acc = 0.f;
  for (int s = 0; s < S; ++s) {
    const float ms = pml[2 * s];
    const float sw = (ms == -INFINITY) ? 0.f : __expf(ms - M);
    L = fmaf(pml[2 * s + 1], sw, L);
    acc = fmaf(po[(long)s * D], sw, acc);
  }
  const float inv = (L > 0.f) ? 1.f / L : 0.f;
  out[row * D + d] = f2bf(acc * inv);
}

constexpr int BLOCK_APP = 256;

// Work item = one 8-wide vec of the first half of one head row and its
// partner in the second half, as qkv_rope_kernel.
__global__ void qkv_rope_append_kernel(
    const bf16x8* __restrict__ qkv, bf16x8* __restrict__ q,
    bf16x8* __restrict__ kcache, bf16x8* __restrict__ vcache,
    const float* __restrict__ tab_cos, const float* __restrict__ tab_sin,
    const int* __restrict__ pos, int B, int Tmax, int Hq, int Hkv,
    int hv /* (D/2)/8 */) {
  const int heads_total = Hq + 2 * Hkv;
  const int dv8 = hv * 2;  // vecs per head (D/8)
  const long nwork = (long)B * heads_total * hv;
  for (long i = (long)blockIdx.x * BLOCK_APP + threadIdx.x; i < nwork;
       i += (long)gridDim.x * BLOCK_APP) {
    const long rowh = i / hv;                 // b*heads_total + h
    const int c = (int)(i - rowh * hv);
    const int b = (int)(rowh / heads_total);
    const int h = (int)(rowh - (long)b * heads_total);
    const int p = pos[b];
    const bool live = p >= 0 && p < Tmax;
    bf16x8* dst;
    bool rot;
    if (h < Hq) {
      dst = q + ((long)b * Hq + h) * dv8;
      rot = true;
      if (!live) {  // a finished sequence: zero q row, caches untouched
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
      dst = (isk ? kcache : vcache) +
            (((long)b * Tmax + p) * Hkv + hh) * dv8;
      rot = isk;
    }
    const bf16x8* src = qkv + rowh * dv8;
    const bf16x8 x1 = src[c];
    const bf16x8 x2 = src[c + hv];
    if (rot) {
      const float* cosr = tab_cos + (long)p * (hv * 8);
      const float* sinr = tab_sin + (long)p * (hv * 8);
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
void launch_ragged(const void* q, const void* k, const void* v,
                   const int* lens, void* out, float* ws, int B, int Tmax,
                   int Hkv, int num_splits, int chunk, hipStream_t stream) {
  dim3 grid(Hkv, B, num_splits);
  const float scale = 1.f / sqrtf((float)D);
  attn_decode_ragged_kernel<D, R><<<grid, NTH_RAG, 0, stream>>>(
      (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, lens,
      (bf16_t*)out, ws, Tmax, Hkv, chunk, scale);
}

template <int D>
bool launch_ragged_r(int R, const void* q, const void* k, const void* v,
                     const int* lens, void* out, float* ws, int B, int Tmax,
                     int Hkv, int num_splits, int chunk, hipStream_t stream) {
  switch (R) {
    case 1: launch_ragged<D, 1>(q, k, v, lens, out, ws, B, Tmax, Hkv,
                                num_splits, chunk, stream); return true;
    case 2: launch_ragged<D, 2>(q, k, v, lens, out, ws, B, Tmax, Hkv,
                                num_splits, chunk, stream); return true;
    case 4: launch_ragged<D, 4>(q, k, v, lens, out, ws, B, Tmax, Hkv,
                                num_splits, chunk, stream); return true;
    case 8: launch_ragged<D, 8>(q, k, v, lens, out, ws, B, Tmax, Hkv,
                                num_splits, chunk, stream); return true;
    default: return false;
  }
}

}  // namespace

extern "C" {

// ws: fp32, B*Hq*num_splits*(D+2) elements; unused when num_splits == 1.
hipError_t tok_attn_decode_ragged(const void* q, const void* k, const void* v,
                                  const int* lens, void* out, float* ws,
                                  int B, int Tmax, int Hq, int Hkv, int D,
                                  int num_splits, int chunk,
                                  hipStream_t stream) {
  if (Hkv < 1 || Hq % Hkv != 0 || num_splits < 1 || chunk < 1 ||
      (long)num_splits * chunk < Tmax)
    return hipErrorInvalidValue;
  const int R = Hq / Hkv;
  bool ok = false;
  if (D == 128)
    ok = launch_ragged_r<128>(R, q, k, v, lens, out, ws, B, Tmax, Hkv,
                              num_splits, chunk, stream);
  else if (D == 64)
    ok = launch_ragged_r<64>(R, q, k, v, lens, out, ws, B, Tmax, Hkv,
                             num_splits, chunk, stream);
  if (!ok) return hipErrorInvalidValue;
  HIP_CHECK(hipGetLastError());
  if (num_splits > 1) {
    attn_decode_ragged_combine<<<dim3(Hq, B), D, 0, stream>>>(
        ws, (bf16_t*)out, num_splits, D);
    HIP_CHECK(hipGetLastError());
  }
  return hipSuccess;
}

hipError_t tok_qkv_rope_append(const void* qkv, void* q, void* kcache,
                               void* vcache, const float* cos_tab,
                               const float* sin_tab, const int* pos, int B,
                               int Tmax, int Hq, int Hkv, int D,
                               hipStream_t stream) {
  const int hv = (D / 2) / 8;
  const long nwork = (long)B * (Hq + 2 * Hkv) * hv;
  long grid = (nwork + BLOCK_APP - 1) / BLOCK_APP;
  if (grid > 8192) grid = 8192;
  if (grid < 1) grid = 1;
  qkv_rope_append_kernel<<<(int)grid, BLOCK_APP, 0, stream>>>(
      (const bf16x8*)qkv, (bf16x8*)q, (bf16x8*)kcache, (bf16x8*)vcache,
      cos_tab, sin_tab, pos, B, Tmax, Hq, Hkv, hv);
  return hipGetLastError();
}
}
