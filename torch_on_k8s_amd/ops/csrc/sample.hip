// Fused temperature / top-k / top-p token sampler for MI355X (gfx950).
//
//   sample_tokens_kernel   grid (B), 1024 threads, one block per logits row
//     logits [B,V] bf16 (unit stride in V, any row stride, any alignment);
//     temperature/top_p fp32 [B], top_k int32 [B], seed int64 [B], counter
//     int32 or int64 [B], optional u fp32 [B]; all on the device, none read
//     by the host, and the grid depends on B alone: capturable, and a
//     replay follows new contents.
//
// A logit is mapped to a 16-bit key that orders as the floats do (-0 -> +0).
// Temperature keeps the order, so both thresholds live in key space:
//
//   P0     one pass: max key and the lowest index that holds it (one packed
//          integer max). A greedy row (T <= 0) ends here.
//   sweep  only with top-k or top-p active. Key space is walked in
//          descending order in two halves of 32768 keys (a 128 KiB count
//          histogram in LDS, integer atomics only). Thread t owns 32
//          consecutive keys; a block scan in thread order gives every
//          thread the count and the mass  sum(count * exp(z(key)))  above
//          it. The thread in which the count reaches k finds the k-th key
//          and M, the mass of the top-k survivors; every thread's mass
//          prefix is kept (2048 floats). The second half is skipped when
//          the k-th key lies in the first. Without top-k, M is the whole
//          mass: one more pass sums it first, and the second half is
//          skipped when the first already holds top_p * M.
//   top-p  the last group of 32 keys whose mass prefix is below top_p * M
//          holds the cut; its 32 counts are taken from the histogram, or
//          recounted in one more pass if that half has been overwritten.
//   draw   kept = value >= the threshold key's value (a float compare; the
//          keys order as the values do). The row is cut into tiles of 512
//          consecutive elements, one wave per tile; a tile's mass is the
//          last lane of a wave scan. Wave 0 scans the tile masses, takes
//          u from Philox4x32-10 (or from `u`), finds the tile in which the
//          running mass passes u * M_kept and rescans that tile alone for
//          the first index with C_i > u * M_kept. If rounding leaves none:
//          the last kept index whose mass is not 0.
//
// Every sum has a fixed order (serial per lane, shuffle scan per wave, wave
// order per block) and the only atomics are integer ones, so the token is
// a function of the row's contents alone. Every loop is bounded by V or by
// the key width. Rows are read with 16-byte loads at 16-byte-aligned
// addresses, four in flight per lane; the elements before the first and
// after the last aligned vector of a row are read one by one.
//
// Resources (hipcc -O3 --offload-arch=gfx950,
// -Rpass-analysis=kernel-resource-usage; scratch 0 B):
//   kernel                 VGPR  SGPR  LDS B    waves/SIMD
//   sample_tokens_kernel     80   106  147920   4 (one block per CU, by LDS)
// Measured in profiles/sample.log: a pass over 128256 logits takes about
// 13 us on the row's one CU and is VALU time, not load latency.
#include "common.h"

#include <atomic>
#include <cfloat>

namespace {

constexpr int NTH_S = 1024;
constexpr int NW_S = NTH_S / WAVE;        // 16
constexpr int HALF_KEYS = 32768;          // keys per sweep half
constexpr int KEYS_PER_THREAD = HALF_KEYS / NTH_S;  // 32
constexpr int NGROUPS = 2 * NTH_S;        // groups of 32 keys in key space
constexpr int TILE = WAVE * 8;            // elements per draw tile
constexpr int MAX_TILES = 2048;           // V <= 2^20
constexpr int UNROLL = 4;                 // 16-byte loads in flight per lane
constexpr int MAX_DEVICES = 64;           // GPUs one process may launch on

struct SampleShared {
  unsigned int hist[HALF_KEYS];           // [j][t]: key j of thread t
  float prefix[NGROUPS];                  // mass above each group of 32 keys
  float tile_sum[MAX_TILES];
  unsigned int mini[KEYS_PER_THREAD];
  unsigned long long wmax[NW_S];
  int wcnt[NW_S];
  float wmass[NW_S];
  int wint[NW_S];
  int k_pos;       // position (0xFFFF - key) of the k-th largest key
  float k_mass;    // mass of the top-k survivors
  int k_found;
  int last_kept;
};

// bf16 bits -> key that orders as the values do; -0 joins +0
DEVINL unsigned int sort_key(unsigned int b) {
  if ((b & 0x7FFFu) == 0) b = 0;
  return (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
}

DEVINL float key_value(unsigned int k) {
  const unsigned int b = (k & 0x8000u) ? (k & 0x7FFFu) : (~k & 0xFFFFu);
  return bfbits2f((uint16_t)b);
}

// exp((l - max) / T); a logit of -inf gives 0
DEVINL float mass_of(float val, float maxv, float inv_t) {
  return __expf((val - maxv) * inv_t);
}

// The 8 elements of aligned vector pv of a row whose first element sits
// `off` elements after a 16-byte boundary. Elements outside the row read
// as 0 and are masked by the caller through their index.
DEVINL bf16x8 load_vec(const uint16_t* row, int V, int off, int pv) {
  const int i0 = pv * 8 - off;
  bf16x8 r;
  if (i0 >= 0 && i0 + 8 <= V) {
    r = *reinterpret_cast<const bf16x8*>(row + i0);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = i0 + j;
      r.h[j] = (i >= 0 && i < V) ? row[i] : (uint16_t)0;
    }
  }
  return r;
}

// f(index, bits) for every element of the row, in no particular order:
// U aligned 16-byte loads per thread are issued before the first is used
// (one pass is a few dependent round trips to L2, not sixteen); the up to 7
// elements before the first aligned vector and after the last go one by
// one. A slot past the end reloads the thread's first vector and is skipped.
template <int U, class F>
DEVINL void for_row(const uint16_t* row, int V, int off, int tid, F f) {
  const int head = min((8 - off) & 7, V);
  const int nbody = (V - head) >> 3;
  const bf16x8* body = reinterpret_cast<const bf16x8*>(row + head);
  for (int base = tid; base < nbody; base += U * NTH_S) {
    bf16x8 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int pv = base + u * NTH_S;
      v[u] = body[pv < nbody ? pv : base];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int pv = base + u * NTH_S;
      if (pv < nbody) {
#pragma unroll
        for (int j = 0; j < 8; ++j) f(head + pv * 8 + j, v[u].h[j]);
      }
    }
  }
  if (tid < head) f(tid, row[tid]);
  const int t = head + nbody * 8 + tid;
  if (t < V) f(t, row[t]);
}

DEVINL float wave_scan_f(float x, int lane) {
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const float y = __shfl_up(x, d, WAVE);
    if (lane >= d) x += y;
  }
  return x;
}

// the inclusive scan's value one lane down: the exclusive prefix, without
// the rounding of (inclusive - own)
DEVINL float lane_exclusive(float incl, int lane) {
  const float y = __shfl_up(incl, 1, WAVE);
  return lane == 0 ? 0.f : y;
}

DEVINL int wave_scan_i(int x, int lane) {
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const int y = __shfl_up(x, d, WAVE);
    if (lane >= d) x += y;
  }
  return x;
}

DEVINL int wave_max_i(int x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = max(x, __shfl_xor(x, off, WAVE));
  return x;
}

DEVINL int wave_min_i(int x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = min(x, __shfl_xor(x, off, WAVE));
  return x;
}

// block-wide max of an int; every thread gets it. One barrier pair.
DEVINL int block_max_i(int x, int* scratch) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  x = wave_max_i(x);
  __syncthreads();
  if (lane == 0) scratch[wid] = x;
  __syncthreads();
  int m = scratch[0];
#pragma unroll
  for (int w = 1; w < NW_S; ++w) m = max(m, scratch[w]);
  return m;
}

DEVINL void philox_round(uint32_t c[4], uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
  const uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
  const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
  c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
}

// first output word of Philox4x32-10
DEVINL uint32_t philox_first(uint64_t seed, uint64_t counter) {
  uint32_t c[4] = {(uint32_t)counter, (uint32_t)(counter >> 32), 0u, 0u};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c[0];
}

__global__ __launch_bounds__(NTH_S) void sample_tokens_kernel(
    const uint16_t* __restrict__ logits, long row_stride,
    const float* __restrict__ temperature, const int* __restrict__ top_k,
    const float* __restrict__ top_p, const long long* __restrict__ seed,
    const void* __restrict__ counter, int counter_is_64,
    const float* __restrict__ u_opt, long long* __restrict__ out, int V) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  SampleShared& sh = *reinterpret_cast<SampleShared*>(smem_raw);

  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint16_t* row = logits + (long)b * row_stride;
  const int off = (int)((reinterpret_cast<uintptr_t>(row) & 15) >> 1);
  const int nvec = (off + V + 7) >> 3;    // aligned vectors that touch the row

  // ---- P0: max key and the lowest index that holds it --------------------
  unsigned long long best = 0;            // key << 32 | ~index
  for_row<UNROLL>(row, V, off, tid, [&](int i, uint16_t bits) {
    const unsigned long long c = ((unsigned long long)sort_key(bits) << 32) |
                                 (0xFFFFFFFFu - (unsigned)i);
    best = c > best ? c : best;
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long y = __shfl_xor(best, o, WAVE);
    best = y > best ? y : best;
  }
  if (lane == 0) sh.wmax[wid] = best;
  if (tid == 0) {
    sh.k_found = 0;
    sh.last_kept = -1;
  }
  __syncthreads();
  best = sh.wmax[0];
#pragma unroll
  for (int w = 1; w < NW_S; ++w) best = sh.wmax[w] > best ? sh.wmax[w] : best;
  const unsigned int max_key = (unsigned int)(best >> 32);
  const int arg_max = (int)(0xFFFFFFFFu - (unsigned int)best);

  const float T = temperature[b];
  if (!(T > 0.f)) {                       // greedy row (block-uniform)
    if (tid == 0) out[b] = min(max(arg_max, 0), V - 1);
    return;
  }
  // a subnormal T would make 1/T infinite and the maximum's mass 0 * inf;
  // at FLT_MIN the masses below the maximum are already 0, the limit wanted
  const float inv_t = 1.f / fmaxf(T, FLT_MIN);
  const float maxv = key_value(max_key);
  const int max_pos = 0xFFFF - (int)max_key;
  const int kk = top_k[b];
  const float pp = top_p[b];
  const bool k_on = kk > 0 && kk < V;
  const bool p_on = pp < 1.f;

  int thr_pos = 0xFFFF;                   // keep key >= 0xFFFF - thr_pos

  if (k_on || p_on) {
    // top-p on the unfiltered row: M is the whole mass, summed here in one
    // pass (lane, butterfly, waves in order) so that the sweep can stop in
    // the half that holds the cut instead of walking all of key space
    const bool p_alone = !k_on;
    float m_all = 0.f;
    if (p_alone) {
      float s = 0.f;
      for_row<UNROLL>(row, V, off, tid, [&](int, uint16_t bits) {
        s += mass_of(bfbits2f(bits), maxv, inv_t);
      });
      s = wave_reduce_sum(s);
      if (lane == 0) sh.wmass[wid] = s;
      __syncthreads();
      for (int w = 0; w < NW_S; ++w) m_all += sh.wmass[w];
      __syncthreads();                    // wmass is the sweep's too
    }

    // ---- sweep: counts and masses over key space, descending ------------
    int carry_cnt = 0;
    float carry_mass = 0.f;
    int last_half = 0;
    for (int half = 0; half < 2; ++half) {
      last_half = half;
      for (int i = tid; i < HALF_KEYS; i += NTH_S) sh.hist[i] = 0;
      __syncthreads();
      for_row<UNROLL>(row, V, off, tid, [&](int, uint16_t bits) {
        const int pos = 0xFFFF - (int)sort_key(bits);
        if ((pos >> 15) == half) {
          const int q = pos & (HALF_KEYS - 1);
          atomicAdd(&sh.hist[(q & 31) * NTH_S + (q >> 5)], 1u);
        }
      });
      __syncthreads();
      // thread tid owns positions half*32768 + tid*32 + [0, 32)
      const int pos0 = half * HALF_KEYS + tid * KEYS_PER_THREAD;
      int cl = 0;
      float ml = 0.f;
      for (int j = 0; j < KEYS_PER_THREAD; ++j) {
        const unsigned int n = sh.hist[j * NTH_S + tid];
        if (n) {
          cl += (int)n;
          ml = fmaf((float)n,
                    mass_of(key_value(0xFFFFu - (pos0 + j)), maxv, inv_t), ml);
        }
      }
      const int ci = wave_scan_i(cl, lane);
      const float mi = wave_scan_f(ml, lane);
      if (lane == WAVE - 1) {
        sh.wcnt[wid] = ci;
        sh.wmass[wid] = mi;
      }
      __syncthreads();
      int cnt_ex = carry_cnt;
      float mass_ex = carry_mass;
      int tot_cnt = carry_cnt;
      float tot_mass = carry_mass;
      for (int w = 0; w < NW_S; ++w) {
        if (w == wid) {
          cnt_ex = tot_cnt;
          mass_ex = tot_mass;
        }
        tot_cnt += sh.wcnt[w];
        tot_mass += sh.wmass[w];
      }
      cnt_ex += ci - cl;
      mass_ex += lane_exclusive(mi, lane);
      sh.prefix[half * NTH_S + tid] = mass_ex;
      if (k_on && cnt_ex < kk && kk <= cnt_ex + cl) {   // exactly one thread
        int c2 = cnt_ex;
        float m2 = mass_ex;
        for (int j = 0; j < KEYS_PER_THREAD; ++j) {
          const unsigned int n = sh.hist[j * NTH_S + tid];
          if (n) {
            c2 += (int)n;
            m2 = fmaf((float)n,
                      mass_of(key_value(0xFFFFu - (pos0 + j)), maxv, inv_t),
                      m2);
            if (c2 >= kk) {
              sh.k_pos = pos0 + j;
              sh.k_mass = m2;
              sh.k_found = 1;
              break;
            }
          }
        }
      }
      carry_cnt = tot_cnt;
      carry_mass = tot_mass;
      __syncthreads();
      if (sh.k_found) break;              // block-uniform, as the next
      if (p_alone && carry_cnt > 0 && carry_mass >= pp * m_all) break;
    }
    const int k_pos = sh.k_found ? sh.k_pos : 0xFFFF;
    const float M = sh.k_found ? sh.k_mass : m_all;
    thr_pos = k_pos;

    if (p_on) {
      // ---- top-p: the group of 32 keys that holds the cut ---------------
      const float target = pp * M;
      const int g_hi = min(k_pos >> 5, (last_half + 1) * NTH_S - 1);
      int g = max_pos >> 5;
      for (int h = 0; h <= last_half; ++h) {
        const int gi = h * NTH_S + tid;
        if (gi <= g_hi && sh.prefix[gi] < target) g = max(g, gi);
      }
      g = block_max_i(g, sh.wint);
      g = min(g, g_hi);
      if ((g >> 10) == last_half) {
        if (tid < KEYS_PER_THREAD) sh.mini[tid] = sh.hist[tid * NTH_S + (g & (NTH_S - 1))];
      } else {                            // that half is gone: recount 32 keys
        if (tid < KEYS_PER_THREAD) sh.mini[tid] = 0;
        __syncthreads();
        for_row<UNROLL>(row, V, off, tid, [&](int, uint16_t bits) {
          const int pos = 0xFFFF - (int)sort_key(bits);
          if ((pos >> 5) == g) atomicAdd(&sh.mini[pos & 31], 1u);
        });
      }
      __syncthreads();
      // every thread walks the same 32 counts: no broadcast needed
      float m2 = sh.prefix[g];
      int p_pos = min(g * 32 + 31, k_pos);
      for (int j = 0; j < KEYS_PER_THREAD; ++j) {
        const int pos = g * 32 + j;
        if (pos > k_pos) break;
        const unsigned int n = sh.mini[j];
        if (n) {
          m2 = fmaf((float)n, mass_of(key_value(0xFFFFu - pos), maxv, inv_t),
                    m2);
          if (m2 >= target) {
            p_pos = pos;
            break;
          }
        }
      }
      thr_pos = min(k_pos, p_pos);
    }
  }
  // Keys order as the values do, so kept = (value >= threshold value): a
  // float compare per element instead of a key. Keys at or below -inf's
  // (no filter) keep every number.
  const unsigned int thr_key = 0xFFFFu - (unsigned int)thr_pos;
  const float thr_val = thr_key <= 0x007Fu ? -INFINITY : key_value(thr_key);

  // ---- draw: tile masses in index order ----------------------------------
  const int ntiles = (nvec + WAVE - 1) / WAVE;
  int my_last = -1;
  for (int t0 = wid; t0 < ntiles; t0 += UNROLL * NW_S) {
    bf16x8 v[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {      // all loads first
      const int pv = (t0 + u * NW_S) * WAVE + lane;
      v[u] = load_vec(row, V, off, pv < nvec ? pv : t0 * WAVE);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int t = t0 + u * NW_S;          // wave-uniform
      if (t >= ntiles) break;
      const int pv = t * WAVE + lane;
      float s = 0.f;
      if (pv < nvec) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int i = pv * 8 - off + j;
          const float val = bfbits2f(v[u].h[j]);
          if ((unsigned)i < (unsigned)V && val >= thr_val) {
            const float m = mass_of(val, maxv, inv_t);
            s += m;
            if (m > 0.f) my_last = i;      // a -inf logit is never returned
          }
        }
      }
      s = wave_scan_f(s, lane);
      if (lane == WAVE - 1) sh.tile_sum[t] = s;
    }
  }
  my_last = wave_max_i(my_last);
  if (lane == 0 && my_last >= 0) atomicMax(&sh.last_kept, my_last);
  __syncthreads();
  if (wid != 0) return;

  // wave 0: scan the tile masses, lane l owns tiles [l*per, (l+1)*per)
  const int per = (ntiles + WAVE - 1) / WAVE;
  float ls = 0.f;
  for (int j = 0; j < per; ++j) {
    const int t = lane * per + j;
    if (t < ntiles) ls += sh.tile_sum[t];
  }
  const float incl = wave_scan_f(ls, lane);
  const float total = __shfl(incl, WAVE - 1, WAVE);
  float u;
  if (u_opt) {
    u = u_opt[b];
  } else {
    const uint64_t ctr = counter_is_64
        ? (uint64_t)reinterpret_cast<const long long*>(counter)[b]
        : (uint64_t)(long long)reinterpret_cast<const int*>(counter)[b];
    u = (float)(philox_first((uint64_t)seed[b], ctr) >> 8) * 0x1p-24f;
  }
  const float target = u * total;
  int hit = 0x7FFFFFFF;                   // first tile whose prefix passes
  float hit_ex = 0.f;
  {
    float run = lane_exclusive(incl, lane);
    for (int j = 0; j < per; ++j) {
      const int t = lane * per + j;
      if (t < ntiles) {
        const float nxt = run + sh.tile_sum[t];
        if (nxt > target && hit == 0x7FFFFFFF) {
          hit = t;
          hit_ex = run;
        }
        run = nxt;
      }
    }
  }
  const int tile = wave_min_i(hit);
  int result = sh.last_kept;
  if (tile != 0x7FFFFFFF) {
    // the owning lane's exclusive prefix, to every lane
    const int owner = tile / per;
    const float tile_ex = __shfl(hit_ex, owner, WAVE);
    const int pv = tile * WAVE + lane;
    float m[8];
    int idx_last = -1;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = 0.f;
    if (pv < nvec) {
      const bf16x8 v = load_vec(row, V, off, pv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = pv * 8 - off + j;
        const float val = bfbits2f(v.h[j]);
        if ((unsigned)i < (unsigned)V && val >= thr_val) {
          m[j] = mass_of(val, maxv, inv_t);
          s += m[j];
          if (m[j] > 0.f) idx_last = i;
        }
      }
    }
    const float lane_ex = lane_exclusive(wave_scan_f(s, lane), lane);
    int found = 0x7FFFFFFF;
    float run = lane_ex;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // m[j] > 0 only for kept elements inside the row
      run += m[j];
      if (m[j] > 0.f && tile_ex + run > target && found == 0x7FFFFFFF)
        found = pv * 8 - off + j;
    }
    found = wave_min_i(found);
    idx_last = wave_max_i(idx_last);
    result = (found != 0x7FFFFFFF) ? found : idx_last;
  }
  if (result < 0) result = arg_max;
  if (lane == 0) out[b] = min(max(result, 0), V - 1);
}

}  // namespace

extern "C" {

int tok_sample_max_vocab() { return MAX_TILES * TILE - 8; }

// One block per row. counter is int32 or int64 ([B]); u_opt may be null.
hipError_t tok_sample_tokens(const void* logits, long row_stride,
                             const float* temperature, const int* top_k,
                             const float* top_p, const long long* seed,
                             const void* counter, int counter_is_64,
                             const float* u_opt, long long* out, int B, int V,
                             hipStream_t stream) {
  if (B < 1 || V < 1 || V > tok_sample_max_vocab())
    return hipErrorInvalidValue;
  // 147 KiB of LDS needs the opt-in, once per device
  static std::atomic<bool> attr_set[MAX_DEVICES];
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= MAX_DEVICES) return hipErrorInvalidDevice;
  if (!attr_set[dev].load(std::memory_order_acquire)) {
    HIP_CHECK(hipFuncSetAttribute(
        reinterpret_cast<const void*>(sample_tokens_kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)sizeof(SampleShared)));
    attr_set[dev].store(true, std::memory_order_release);
  }
  sample_tokens_kernel<<<B, NTH_S, sizeof(SampleShared), stream>>>(
      (const uint16_t*)logits, row_stride, temperature, top_k, top_p, seed,
      counter, counter_is_64, u_opt, out, V);
  return hipGetLastError();
}
}
