// Chunked ragged prefill for MI355X (gfx950): Tq new tokens per sequence,
// causal among themselves, against a ragged KV-cache prefix; and the
// multi-token append that goes with it.
//
//   attn_extend_kernel<D, R>   grid (Hkv * ceil(Tq*R/64), B, num_splits), 256 thr
//     q [B,Tq,Hq,D], kcache/vcache [B,Tmax,Hkv,D] (the new tokens' K/V already
//     appended), lens/qlens [B] int32 on the device.
//     The row layout of kt_attn (attn_kv_tile.h: the work split, operand
//     layouts, LDS image, bank argument, softmax and epilogue) over a
//     contiguous cache: tile t of split z is cache rows kbeg + 64t .. + 63 of
//     one kv head, Hkv*D*2 bytes apart, clamped to kend - 1; nothing is read
//     ahead between tiles.
//
//   qkv_rope_append_chunk_kernel   grid-stride, 256 threads
//     qkv [B,Tq,(Hq+2Hkv)*D]: token i of sequence b is rotated at pos[b] + i
//     and its k, v written to cache[b, pos[b] + i]; live iff i < qlens[b] and
//     0 <= pos[b] + i < Tmax; a dead token gets a zero q row and writes
//     nothing. Per element as qkv_rope_append_kernel: fp32, two products and
//     an add. The four multi-token rope appends (this one, the paged one and
//     the two of kv_fp8.hip) stay four bodies: the compiler contracts
//     a*cs - b*sn into one fma and picks the product to fuse by the code
//     around it, so a shared body changed the last bit of a few outputs.
//
// Resources (hipcc -O3 --offload-arch=gfx950,
// -Rpass-analysis=kernel-resource-usage; scratch is 0 B everywhere):
//   kernel                         VGPR  SGPR  LDS B  waves/SIMD
//   attn_extend_kernel<128,1>       141    54  65536  2
//   attn_extend_kernel<128,2|4|8>   141    56  65536  2
//   attn_extend_kernel<64,1>         94    54  32768  5
//   attn_extend_kernel<64,2|4|8>     94    56  32768  5
//   qkv_rope_append_chunk_kernel     51    70      0  8
// (waves/SIMD is the register figure; LDS allows two blocks = 2 waves/SIMD at
// D = 128 and five blocks at D = 64.)
#include "attn_kv_tile.h"

extern "C" hipError_t tok_attn_ragged_combine(const float* ws, void* out,
                                              int rows, int Hq, int D,
                                              int num_splits,
                                              hipStream_t stream);

namespace {

template <int D>
struct ContigSrc {
  const bf16_t *kc, *vc;
  int tmax;
  // of the block
  const char *kbase, *vbase;
  uint32_t row_bytes;  // between cache rows
  int kbeg, klast, d_row, d_ch;

  DEVINL ContigSrc(const bf16_t* k, const bf16_t* v, int Tmax)
      : kc(k), vc(v), tmax(Tmax) {}
  DEVINL int Tmax() const { return tmax; }
  DEVINL void begin(int b, int hkv, int Hkv, int kbeg_, int kend, int d_row_,
                    int d_ch_) {
    row_bytes = (uint32_t)Hkv * D * 2;
    const long head_off = ((long)b * tmax * Hkv + hkv) * D;
    kbase = reinterpret_cast<const char*>(kc + head_off);
    vbase = reinterpret_cast<const char*>(vc + head_off);
    kbeg = kbeg_, klast = kend - 1, d_row = d_row_, d_ch = d_ch_;
  }
  // One K and one V tile, keys clamped to klast, into the pair of tiles at
  // LDS address dst (wave part included).
  DEVINL void issue(int tile, uint32_t dst) const {
    constexpr int TILE = KT_PAGE * D * 2, NJ = TILE / 4096;
    constexpr int RPS = 4096 / (D * 2);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int key = min(kbeg + tile * KT_PAGE + j * RPS + d_row, klast);
      const uint32_t voff = (uint32_t)key * row_bytes + d_ch * 16;
      kt_glds16(voff, kbase, dst + j * 4096);
      kt_glds16(voff, vbase, dst + TILE + j * 4096);
    }
  }
  DEVINL void prefetch(int) {}
};

template <int D, int R>
KT_KERNEL __launch_bounds__(KT_NTH, 2) void attn_extend_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ kc,
    const bf16_t* __restrict__ vc, const int* __restrict__ lens,
    const int* __restrict__ qlens, bf16_t* __restrict__ out,
    float* __restrict__ ws, int Tq, int Tmax, int Hkv, int MT, int chunk,
    float scale) {
  kt_attn<D, R, false>(ContigSrc<D>(kc, vc, Tmax), q, lens, qlens, out, ws, Tq,
                       Hkv, MT, chunk, scale);
}

// Work item = one 8-wide vec of the first half of one head row of one token
// and its partner in the second half, as qkv_rope_append_kernel.
KT_KERNEL void qkv_rope_append_chunk_kernel(
    const bf16x8* __restrict__ qkv, bf16x8* __restrict__ q,
    bf16x8* __restrict__ kcache, bf16x8* __restrict__ vcache,
    const float* __restrict__ tab_cos, const float* __restrict__ tab_sin,
    const int* __restrict__ pos, const int* __restrict__ qlens, int B, int Tq,
    int Tmax, int Hq, int Hkv, int hv /* (D/2)/8 */) {
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

}  // namespace

extern "C" {

// ws: fp32, B*Tq*Hq*num_splits*(D+2) elements; unused when num_splits == 1.
hipError_t tok_attn_extend(const void* q, const void* k, const void* v,
                           const int* lens, const int* qlens, void* out,
                           float* ws, int B, int Tq, int Tmax, int Hq, int Hkv,
                           int D, int num_splits, int chunk,
                           hipStream_t stream) {
  if (Hkv < 1 || Hq % Hkv != 0 || Tq < 1 || num_splits < 1 ||
      chunk < KT_PAGE || chunk % KT_PAGE != 0 ||
      (long)num_splits * chunk < Tmax ||
      (long)Tmax * Hkv * D * 2 >= (1L << 31))
    return hipErrorInvalidValue;
  const bool ok = kt_dispatch(D, Hq / Hkv, [&](auto d, auto r) {
    constexpr int DD = decltype(d)::value, R = decltype(r)::value;
    const int MT = (Tq * R + 63) / 64;  // the row layout only
    dim3 grid(Hkv * MT, B, num_splits);
    const float scale = 1.f / sqrtf((float)DD);
    attn_extend_kernel<DD, R><<<grid, KT_NTH, 0, stream>>>(
        (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, lens, qlens,
        (bf16_t*)out, ws, Tq, Tmax, Hkv, MT, chunk, scale);
  });
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
  const int grid = kt_append_grid((long)B * Tq * (Hq + 2 * Hkv) * hv);
  qkv_rope_append_chunk_kernel<<<grid, KT_NTH, 0, stream>>>(
      (const bf16x8*)qkv, (bf16x8*)q, (bf16x8*)kcache, (bf16x8*)vcache,
      cos_tab, sin_tab, pos, qlens, B, Tq, Tmax, Hq, Hkv, hv);
  return hipGetLastError();
}
}
