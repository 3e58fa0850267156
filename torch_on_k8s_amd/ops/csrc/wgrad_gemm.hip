// Weight-gradient GEMM for gfx950: C[N,K] (+)= dy[M,N]^T · x[M,K].
//
// dy and x are both row-major and the contraction runs over their rows
// (tokens), the layout a BLAS "NT" call serves worst. Here both operands are
// staged as they lie in memory, [token][column], by 16-byte global->LDS DMA,
// and handed to the MFMA with the token index along the register by the
// transposed LDS read (ds_read_b64_tr_b16). The result is written once,
// with the old C added in fp32 before the single rounding to bf16, so the
// caller needs neither a temporary nor a separate accumulate pass.
//
// Geometry: 256 x 256 output tile, 64 tokens per step, 8 waves (2 x 4), each
// wave 128 x 64 of the tile as 8 x 4 accumulators of mfma_f32_16x16x32_bf16.
//
// LDS: one array. A step's operands are four units of [64 tokens][128
// columns] (16 KiB, 256-byte rows), two buffers each, 128 KiB in all:
//   A_lo / A_hi = dy columns 0..127 / 128..255 of the tile,
//   B_lo / B_hi = x  columns 0..127 / 128..255 of the tile.
// Wave (wr, wc) owns output rows 64wr..64wr+63 of BOTH A units and output
// columns 32wc..32wc+31 of BOTH B units, so that a unit is exactly what one
// phase reads and can be restaged as soon as that phase is over.
//
// Unit image: chunk ch (16 B) of row r sits at 256 r + 16 (ch ^ f(r)),
// f(r) = ((r & 3) << 2) | ((r >> 2) & 3). The DMA writes LDS linearly (wave
// base + 16 lane), so the XOR is applied to the global SOURCE chunk and again
// to the read address. Bank conflicts of a transposed read, by the rule
// "bank = (addr / 4) % 64, conflicts within a 32-lane half": a half is two
// 16-lane groups on rows r0..r0+3 and r0+8..r0+11 (r0 % 4 == 0) of the same
// two chunks 2c, 2c+1; its 16 (row, chunk) pairs land on slots
// (2c + b) ^ (q << 2) ^ t ^ (2 g) for b, g in {0,1}, q in 0..3: bit 0 from
// b, bit 1 from g, bits 2-3 from q: 16 distinct 16-byte slots of the
// 256-byte bank row, 8 bytes per lane: conflict-free, for A and B alike.
//
// Schedule per 64-token tile t in buffer b (4 phases; every phase is
// reads, 2 DMAs, barrier, lgkmcnt(0), 16 MFMAs, barrier):
//   phase 0: read A_lo, B_lo   C[lo][lo]   stage A_hi[b^1] <- tile t+1
//   phase 1: read B_hi         C[lo][hi]   stage A_lo[b]   <- tile t+2
//   phase 2: read A_hi         C[hi][hi]   stage B_lo[b]   <- tile t+2
//   phase 3: --                C[hi][lo]   stage B_hi[b]   <- tile t+2
//            then vmcnt(6) before the phase's first barrier.
// Write-after-read: a unit is restaged at least one phase after its last
// read, and that read was retired by lgkmcnt(0) ahead of the barrier that
// ends its phase. Read-after-write: phase 3's vmcnt(6) leaves only the three
// units just issued in flight, so all of tile t+1 has landed; the barrier
// after it publishes that to every wave and tile t+1 is first read one phase
// later. The count never reaches 0 inside the loop. Source tiles past the
// end are clamped to the last tile: those DMAs land in units nobody reads
// again and keep the counts uniform.
//
// No float atomics and a fixed summation order: results are bitwise
// repeatable and do not depend on the block order.
#include "common.h"

namespace {

using bf16x8v = __attribute__((ext_vector_type(8))) __bf16;
using bf16x4v = __attribute__((ext_vector_type(4))) __bf16;
using i16x4v = __attribute__((ext_vector_type(4))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int WG_TILE = 256;            // output tile edge, both ways
constexpr int WG_BK = 64;               // tokens per step
constexpr int WG_NTH = 512;
constexpr int UNIT_BYTES = 64 * 256;    // [64 tokens][128 columns] bf16
constexpr int BUF_STRIDE = UNIT_BYTES;  // unit u, buffer b at (2u + b) units
constexpr int U_ALO = 0 * 2 * UNIT_BYTES;
constexpr int U_AHI = 1 * 2 * UNIT_BYTES;
constexpr int U_BLO = 2 * 2 * UNIT_BYTES;
constexpr int U_BHI = 3 * 2 * UNIT_BYTES;
constexpr int EPI_LD = 68;              // floats per epilogue row (64 + pad)
constexpr int WG_LDS_BYTES = 8 * 64 * EPI_LD * 4;
static_assert(WG_LDS_BYTES >= 8 * UNIT_BYTES, "epilogue image covers staging");

typedef __attribute__((address_space(3))) i16x4v* lds_tr_ptr;

// 4 tokens x 16 columns per 16-lane group, token index along the register.
DEVINL i16x4v tr_read(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)p);
}

DEVINL bf16x8v frag(i16x4v lo, i16x4v hi) {
  union { i16x4v s[2]; bf16x8v f; } c;
  c.s[0] = lo;
  c.s[1] = hi;
  return c.f;
}

// 16 bytes per lane, global -> LDS: lane i's bytes land at lds_dst + 16 i.
// Source = scalar base + 32-bit lane offset. M0 carries the LDS base and is
// put back; as inline asm the compiler sees no LDS write to order later
// reads behind, the counted waits below do that.
DEVINL void glds16(uint32_t voff, const void* sbase, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_dst)
      : "memory");
}

DEVINL void wg_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

struct WgCtx {
  const char* lds;       // staging base
  uint32_t lds_u32;      // same, as the DMA's 32-bit LDS address + wave part
  uint32_t ra[2][4];     // A read offsets: [token half u][m tile]
  uint32_t rb[2][2];     // B read offsets: [token half u][n tile]
  uint32_t vdy[2], vx[2];  // DMA lane offsets: rows r and r + 32
  const char* dy0;       // dy + n0, tile 0
  const char* x0;        // x + k0, tile 0
  long dy_step, x_step;  // bytes per 64-token tile
  int last;              // T - 1
};

template <int UNIT, int BUF>
DEVINL void stage_unit(const WgCtx& c, const char* src, const uint32_t (&v)[2]) {
  const uint32_t dst = c.lds_u32 + UNIT + BUF * BUF_STRIDE;
  glds16(v[0], src, dst);
  glds16(v[1], src, dst + 8192);
}

template <int UNIT, int BUF>
DEVINL void read_a(const WgCtx& c, bf16x8v (&a)[4][2]) {
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int o = UNIT + BUF * BUF_STRIDE + s * 8192;
      a[mi][s] = frag(tr_read(c.lds + c.ra[0][mi] + o),
                      tr_read(c.lds + c.ra[1][mi] + o));
    }
}

template <int UNIT, int BUF>
DEVINL void read_b(const WgCtx& c, bf16x8v (&b)[2][2]) {
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int o = UNIT + BUF * BUF_STRIDE + s * 8192;
      b[ni][s] = frag(tr_read(c.lds + c.rb[0][ni] + o),
                      tr_read(c.lds + c.rb[1][ni] + o));
    }
}

// barrier, retire this phase's reads, one C quadrant x 64 tokens, barrier
template <int MH, int NH>
DEVINL void mma_quadrant(f32x4 (&acc)[8][4], const bf16x8v (&a)[4][2],
                         const bf16x8v (&b)[2][2]) {
  wg_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        acc[MH * 4 + mi][NH * 2 + ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a[mi][s], b[ni][s], acc[MH * 4 + mi][NH * 2 + ni], 0, 0, 0);
  __builtin_amdgcn_s_setprio(0);
  wg_barrier();
}

template <int BUF>
DEVINL void wgrad_tile(const WgCtx& c, int t, f32x4 (&acc)[8][4]) {
  bf16x8v a[4][2], b0[2][2], b1[2][2];
  const long t1 = min(t + 1, c.last), t2 = min(t + 2, c.last);
  const char* dy1 = c.dy0 + t1 * c.dy_step;
  const char* dy2 = c.dy0 + t2 * c.dy_step;
  const char* x2 = c.x0 + t2 * c.x_step;

  read_a<U_ALO, BUF>(c, a);
  read_b<U_BLO, BUF>(c, b0);
  stage_unit<U_AHI, BUF ^ 1>(c, dy1 + 256, c.vdy);
  mma_quadrant<0, 0>(acc, a, b0);

  read_b<U_BHI, BUF>(c, b1);
  stage_unit<U_ALO, BUF>(c, dy2, c.vdy);
  mma_quadrant<0, 1>(acc, a, b1);

  read_a<U_AHI, BUF>(c, a);
  stage_unit<U_BLO, BUF>(c, x2, c.vx);
  mma_quadrant<1, 1>(acc, a, b1);

  stage_unit<U_BHI, BUF>(c, x2 + 256, c.vx);
  asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  mma_quadrant<1, 0>(acc, a, b0);
}

__global__ __launch_bounds__(WG_NTH, 2) void wgrad_gemm_kernel(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
    bf16_t* __restrict__ C, int T, int N, int K, int accumulate, int group) {
  __shared__ __attribute__((aligned(1024))) char smem[WG_LDS_BYTES];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 2, wc = wid & 3;

  // Block order. XCD r gets the r-th contiguous share of the tile list (a
  // bijection for any block count); inside the list, bands of `group` dy
  // column slabs are walked x slab by x slab, so the blocks in flight on one
  // XCD share few slabs of either operand. group = 1 keeps one dy slab
  // while sweeping every x slab.
  const unsigned TN = N / WG_TILE, TK = K / WG_TILE;
  unsigned w;
  {
    const unsigned nwg = gridDim.x, l = blockIdx.x;
    const unsigned q = nwg >> 3, r = nwg & 7, xcd = l & 7;
    w = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (l >> 3);
  }
  unsigned tn, tk;
  {
    const unsigned per = (unsigned)group * TK;
    const unsigned first = (w / per) * group;
    const unsigned gsz = min(TN - first, (unsigned)group);
    const unsigned rem = w % per;
    tn = first + rem % gsz;
    tk = rem / gsz;
  }
  const long n0 = (long)tn * WG_TILE, k0 = (long)tk * WG_TILE;

  WgCtx c;
  c.lds = smem;
  c.lds_u32 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)
                  smem + wid * 1024;
  c.lds_u32 = __builtin_amdgcn_readfirstlane(c.lds_u32);
  {
    // transposed read: lane 4q+p of group g supplies row 8g + 4u + q,
    // columns 16c + 4p .. 16c + 4p + 3 (chunk 2c + (p >> 1), half p & 1)
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int row = 8 * g + 4 * u + q;
      const int f = (q << 2) | ((2 * g + u) & 3);
      const uint32_t base = 256 * row + 8 * (p & 1);
      const uint32_t xo = 16 * ((p >> 1) ^ f);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        c.ra[u][mi] = base + (xo ^ (32 * (4 * wr + mi)));
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        c.rb[u][ni] = base + (xo ^ (32 * (2 * wc + ni)));
    }
  }
  {
    // DMA: thread t fills LDS bytes 16 t .. 16 t + 15 of a unit's first 32
    // rows (then of its last 32): row t / 16, slot t % 16 = chunk ^ f(row)
    const int row = tid >> 4, slot = tid & 15;
    const int f = ((row & 3) << 2) | ((row >> 2) & 3);
    const uint32_t ch = slot ^ f;
    c.vdy[0] = (uint32_t)row * N * 2 + ch * 16;
    c.vdy[1] = c.vdy[0] + 32u * N * 2;
    c.vx[0] = (uint32_t)row * K * 2 + ch * 16;
    c.vx[1] = c.vx[0] + 32u * K * 2;
  }
  c.dy0 = (const char*)(dy + n0);
  c.x0 = (const char*)(x + k0);
  c.dy_step = (long)WG_BK * N * 2;
  c.x_step = (long)WG_BK * K * 2;
  c.last = T - 1;

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // prologue: tile 0 whole, tile 1 but for A_hi (phase 0 of tile 0 sends it)
  {
    const long t1 = min(1, c.last);
    const char* dy1 = c.dy0 + t1 * c.dy_step;
    const char* x1 = c.x0 + t1 * c.x_step;
    stage_unit<U_ALO, 0>(c, c.dy0, c.vdy);
    stage_unit<U_BLO, 0>(c, c.x0, c.vx);
    stage_unit<U_BHI, 0>(c, c.x0 + 256, c.vx);
    stage_unit<U_AHI, 0>(c, c.dy0 + 256, c.vdy);
    stage_unit<U_ALO, 1>(c, dy1, c.vdy);
    stage_unit<U_BLO, 1>(c, x1, c.vx);
    stage_unit<U_BHI, 1>(c, x1 + 256, c.vx);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    wg_barrier();
  }

  int t = 0;
  for (; t + 1 < T; t += 2) {
    wgrad_tile<0>(c, t, acc);
    wgrad_tile<1>(c, t + 1, acc);
  }
  if (t < T) wgrad_tile<0>(c, t, acc);

  // Epilogue. Every DMA has landed and every read is over before the LDS
  // is reused; from here each wave works in a private [64][EPI_LD] fp32
  // image, one 64-row half of its output at a time, and leaves it by rows:
  // 8 columns per lane, old C added in fp32, one rounding, 16-byte stores.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  float* ep = (float*)smem + wid * 64 * EPI_LD;
  const int fr = lane & 15, fq = lane >> 4;
  const int orow = lane >> 3, ocol = (lane & 7) * 8;
  const long ccol = k0 + (ocol >> 5) * 128 + wc * 32 + (ocol & 31);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          ep[(mi * 16 + fq * 4 + j) * EPI_LD + ni * 16 + fr] =
              acc[h * 4 + mi][ni][j];
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int row = it * 8 + orow;
      const float* src = ep + row * EPI_LD + ocol;
      const f32x4 v0 = *(const f32x4*)src;
      const f32x4 v1 = *(const f32x4*)(src + 4);
      float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
      bf16_t* dst = C + (n0 + h * 128 + wr * 64 + row) * (long)K + ccol;
      if (accumulate) {
        const bf16x8 old = *(const bf16x8*)dst;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += bfbits2f(old.h[e]);
      }
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o.h[e] = f2bfbits(v[e]);
      *(bf16x8*)dst = o;
    }
  }
}

}  // namespace

// C[N,K] = (accumulate ? C : 0) + dy[M,N]^T x[M,K], all bf16 row-major and
// 16-byte aligned; M % 64 == 0, N % 256 == 0, K % 256 == 0. `group` is the
// raster's band height in dy slabs (>= 1). Launches on `stream` only:
// no allocation, copy or sync, so the call can be captured.
extern "C" hipError_t tok_wgrad_gemm(const void* dy, const void* x, void* c,
                                     long M, long N, long K, int accumulate,
                                     int group, hipStream_t stream) {
  if (M < WG_BK || M % WG_BK || N < WG_TILE || N % WG_TILE || K < WG_TILE ||
      K % WG_TILE || group < 1)
    return hipErrorInvalidValue;
  // lane offsets of the DMA are 32-bit: 64 rows of the wider operand
  if (64 * (N > K ? N : K) * 2 >= (1L << 31) || M / WG_BK >= (1L << 30))
    return hipErrorInvalidValue;
  const long tiles = (N / WG_TILE) * (K / WG_TILE);
  if (tiles >= (1L << 30)) return hipErrorInvalidValue;
  if (group > N / WG_TILE) group = (int)(N / WG_TILE);   // one band at most
  wgrad_gemm_kernel<<<dim3((unsigned)tiles), WG_NTH, 0, stream>>>(
      (const bf16_t*)dy, (const bf16_t*)x, (bf16_t*)c, (int)(M / WG_BK),
      (int)N, (int)K, accumulate, group);
  return hipGetLastError();
}
