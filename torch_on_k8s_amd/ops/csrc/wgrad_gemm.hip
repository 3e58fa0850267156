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
// Counted since (profiles/pmc_wgrad.csv): SQ_LDS_BANK_CONFLICT is 1024 cycles
// per block at every token count, the epilogue's fp32 image; none in the loop.
//
// Three schedules compute the same bits: every accumulator sees the same
// MFMAs in the same order (tokens in order, slice s = 0 then s = 1 of a
// tile), the old C is added last, one rounding.
//
// ---- Variant 1 (default): reads under the MFMAs, one barrier per phase ----
// A phase is: barrier, 2 DMAs, 16 MFMAs in 8 pairs (s, mi) with the
// fragment reads of the NEXT use dealt between the pairs, each into the
// registers the pair before it has just freed; then, in three phases of
// four, a counted vmcnt. There is one fragment set (a, b0, b1), as in
// variant 0. The compiler counts lgkmcnt for its own ds_reads, so every MFMA
// waits for exactly the reads it consumes (lgkmcnt(6)/(4) at a phase's head,
// a 14..0 count-down in phase 2); sched_barrier(0) pins the issue order the
// argument below assumes. Per tile t in buffer b (c = b ^ 1):
//   phase 0: C[lo][lo]  stage A_hi[c] <- t+1   read A_lo[b] s=1 (under s=0),
//                                              B_hi[b] (under s=1)  vmcnt(8)
//   phase 1: C[lo][hi]  stage A_lo[b] <- t+2   read A_hi[b], fragment (s, mi)
//                                              after pair (s, mi)
//   phase 2: C[hi][hi]  stage B_lo[b] <- t+2   no reads             vmcnt(8)
//   phase 3: C[hi][lo]  stage B_hi[b] <- t+2   read A_lo[c] s=0 (under s=0),
//                                              B_lo[c] (under and after s=1)
//                                                                   vmcnt(8)
// DMA issue order, two instructions per unit:
//   ... A_lo[c](t+1) B_lo[c](t+1) B_hi[c](t+1) | A_hi[c](t+1) A_lo[b](t+2)
//   B_lo[b](t+2) B_hi[b](t+2) | ...          ( | = first barrier of a tile)
// A vmcnt(8) after a phase's DMAs leaves that unit and the three before it in
// flight: the unit issued four phases earlier has landed in this wave, and
// the barrier that opens the next phase says so of every wave.
//   unit    DMA issue   published by                first read   last read
//   A_hi[b] (t-1).0     vmcnt(8) end t.0, bar t.1   t.1          t.1
//   A_lo[c] (t-1).1     vmcnt(8) end t.2, bar t.3   t.3          (t+1).0
//   B_lo[c] (t-1).2     vmcnt(8) end t.2, bar t.3   t.3          t.3
//   B_hi[c] (t-1).3     vmcnt(8) end t.3, bar (t+1).0  (t+1).0   (t+1).0
// (A_lo and B_lo are waited for together: B_lo is the later of the two.)
// Read-after-write: each first read lies behind the barrier in its row, never
// in the phase of the wait. Write-after-read: a unit is restaged behind a
// barrier that every wave reaches only after MFMAs that consumed its last
// read, and LDS reads return in order, so a consumed fragment means every
// earlier read has left the LDS:
//   A_lo[b] last read t.0, consumed by t.0's s=1 pairs; restaged behind bar t.1
//   B_lo[b] last read (t-1).3, consumed by t.0;          restaged behind bar t.2
//   B_hi[b] last read t.0, consumed by t.1;              restaged behind bar t.3
//   A_hi[b] last read t.1, consumed by t.2;          restaged behind bar (t+1).0
// Prologue: variant 0's seven units and vmcnt(6), barrier, then A_lo[0] s=0
// and B_lo[0] into a and b0; the issue order continues the pattern above, so
// the loop's counts hold from tile 0. The last tile's phase 3 reads a clamped
// tile into fragments nobody uses.
//
// ---- Half blocks (the `split` trailing tiles of the raster) ----
// One block runs per compute unit (136 KiB of LDS), so tiles % units tiles
// would occupy a whole last round. When twice that number still fits one
// round, each such tile is computed by two blocks of 128 x 256 (rows 128 h..),
// placed after all full blocks in the same launch. A half block stages its
// A unit, B_lo and B_hi (at U_ALO, U_BLO, U_BHI, two buffers each), holds 4 x 4
// accumulators and runs two phases per tile. Its spare registers hold a
// second fragment set, so all of tile t+1 is read from buffer c during tile
// t (b = t & 1, c = b ^ 1), and every phase ends with lgkmcnt(0): the reads
// sit under the first half of the MFMAs and have long returned.
//   phase 0: C[h][lo]  stage B_lo[b], B_hi[b] <- t+2   read A[c]   (tile t+1)
//   phase 1: C[h][hi]  stage A[c] <- t+3               read B_lo[c], B_hi[c]
//   both end: lgkmcnt(0), vmcnt(6), and the next phase's barrier follows.
// Issue order: ... A[c](t+1) | B[c](t+1) x2 | A[b](t+2) | B[b](t+2) x2 | ...
// vmcnt(6) at the end of t.0 leaves A[b](t+2) and B[b](t+2) in flight, so
// B[c](t+1) has landed, read in t.1; at the end of t.1 it leaves B[b](t+2) and
// A[c](t+3), so A[b](t+2) has landed, read in (t+1).0: three phases of flight
// each. Write-after-read: the unit a phase restages was read in the phase
// before and retired by that phase's lgkmcnt(0) ahead of the barrier.
//
// ---- Variant 0: the first schedule, kept as it was (A/B and bit reference) --
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
constexpr int WG_DEFAULT_VARIANT = 1;  // profiles/wgrad_v2.log
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

// ---------------------------------------------------------------------------
// Variant 1 and the half blocks. Everything above is variant 0, untouched.
// ---------------------------------------------------------------------------

// One fragment (two transposed reads), pinned behind what was issued before
// it and ahead of what follows: the schedule below is the issue order.
template <int UNIT, int BUF>
DEVINL void read_frag(const WgCtx& c, bf16x8v& f, uint32_t o0, uint32_t o1,
                      int s) {
  const int o = UNIT + BUF * BUF_STRIDE + s * 8192;
  f = frag(tr_read(c.lds + o0 + o), tr_read(c.lds + o1 + o));
  __builtin_amdgcn_sched_barrier(0);
}
template <int UNIT, int BUF>
DEVINL void read_a1(const WgCtx& c, bf16x8v (&a)[4][2], int mi, int s) {
  read_frag<UNIT, BUF>(c, a[mi][s], c.ra[0][mi], c.ra[1][mi], s);
}
// rb carries U_BLO here (wg_setup<true>): the B units lie past the 64 KiB an
// LDS instruction's immediate offset reaches.
template <int UNIT, int BUF>
DEVINL void read_b1(const WgCtx& c, bf16x8v (&b)[2][2], int ni, int s) {
  read_frag<UNIT - U_BLO, BUF>(c, b[ni][s], c.rb[0][ni], c.rb[1][ni], s);
}

// The two MFMAs of (s, mi) of one C quadrant, in variant 0's order.
template <int MH, int NH, int ROWS>
DEVINL void mma_pair(f32x4 (&acc)[ROWS][4], const bf16x8v (&a)[4][2],
                     const bf16x8v (&b)[2][2], int s, int mi) {
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
    acc[MH * 4 + mi][NH * 2 + ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
        a[mi][s], b[ni][s], acc[MH * 4 + mi][NH * 2 + ni], 0, 0, 0);
  __builtin_amdgcn_sched_barrier(0);
}

// lgkmcnt(0) alone, as the builtin: the compiler's own wait counting sees it.
DEVINL void wait_lds_reads() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_sched_barrier(0);
}

DEVINL void phase_open() {
  wg_barrier();
}
DEVINL void mma_open() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_setprio(1);
}
DEVINL void mma_close() {
  __builtin_amdgcn_s_setprio(0);
  __builtin_amdgcn_sched_barrier(0);
}

// Variant 1: one barrier per phase, fragment reads under the MFMAs of the
// phase before their use (hazard argument in the file header). On entry a
// holds A_lo[BUF] slice 0 and b0 all of B_lo[BUF] of tile t (in flight or
// landed in registers); on exit the same of tile t + 1 in BUF ^ 1.
template <int BUF>
DEVINL void wgrad_tile_v1(const WgCtx& c, int t, f32x4 (&acc)[8][4],
                          bf16x8v (&a)[4][2], bf16x8v (&b0)[2][2],
                          bf16x8v (&b1)[2][2]) {
  const long t1 = min(t + 1, c.last), t2 = min(t + 2, c.last);
  const char* dy1 = c.dy0 + t1 * c.dy_step;
  const char* dy2 = c.dy0 + t2 * c.dy_step;
  const char* x2 = c.x0 + t2 * c.x_step;

  // phase 0: C[lo][lo]; reads A_lo slice 1, then B_hi
  phase_open();
  stage_unit<U_AHI, BUF ^ 1>(c, dy1 + 256, c.vdy);
  mma_open();
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    mma_pair<0, 0>(acc, a, b0, 0, mi);
    read_a1<U_ALO, BUF>(c, a, mi, 1);
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    mma_pair<0, 0>(acc, a, b0, 1, mi);
    read_b1<U_BHI, BUF>(c, b1, mi & 1, mi >> 1);
  }
  mma_close();
  asm volatile("s_waitcnt vmcnt(8)" ::: "memory");   // A_hi[BUF] of tile t

  // phase 1: C[lo][hi]; A_hi replaces A_lo fragment by fragment
  phase_open();
  stage_unit<U_ALO, BUF>(c, dy2, c.vdy);
  mma_open();
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      mma_pair<0, 1>(acc, a, b1, s, mi);
      read_a1<U_AHI, BUF>(c, a, mi, s);
    }
  mma_close();

  // phase 2: C[hi][hi]; no reads
  phase_open();
  stage_unit<U_BLO, BUF>(c, x2, c.vx);
  mma_open();
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) mma_pair<1, 1>(acc, a, b1, s, mi);
  mma_close();
  asm volatile("s_waitcnt vmcnt(8)" ::: "memory");   // A_lo, B_lo[BUF ^ 1]

  // phase 3: C[hi][lo]; tile t + 1's A_lo slice 0 and B_lo as a and b0 free
  phase_open();
  stage_unit<U_BHI, BUF>(c, x2 + 256, c.vx);
  mma_open();
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    mma_pair<1, 0>(acc, a, b0, 0, mi);
    read_a1<U_ALO, BUF ^ 1>(c, a, mi, 0);
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    mma_pair<1, 0>(acc, a, b0, 1, mi);
    if (mi < 2) read_b1<U_BLO, BUF ^ 1>(c, b0, mi, 0);
  }
  read_b1<U_BLO, BUF ^ 1>(c, b0, 0, 1);
  read_b1<U_BLO, BUF ^ 1>(c, b0, 1, 1);
  mma_close();
  asm volatile("s_waitcnt vmcnt(8)" ::: "memory");   // B_hi[BUF ^ 1]
}

// Block index in raster order -> tile
DEVINL void wg_raster(unsigned w, unsigned TN, unsigned TK, int group,
                      unsigned& tn, unsigned& tk) {
  const unsigned per = (unsigned)group * TK;
  const unsigned first = (w / per) * group;
  const unsigned gsz = min(TN - first, (unsigned)group);
  const unsigned rem = w % per;
  tn = first + rem % gsz;
  tk = rem / gsz;
}

// Read and DMA lane offsets, as in wgrad_gemm_kernel. `wr` picks the 64-row
// slice of an A unit, `wc` the 32-column slice of a B unit. B_BIASED: rb is
// relative to U_BLO's place instead of the array's start (read_b1).
template <bool B_BIASED>
DEVINL void wg_setup(WgCtx& c, const char* smem, int tid, int wr, int wc,
                     const bf16_t* dy, const bf16_t* x, long n0, long k0,
                     int T, int N, int K) {
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  c.lds = smem;
  c.lds_u32 = (uint32_t)(uintptr_t)(__attribute__((address_space(3)))
                                        const char*)smem + wid * 1024;
  c.lds_u32 = __builtin_amdgcn_readfirstlane(c.lds_u32);
  {
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
        c.rb[u][ni] = base + (xo ^ (32 * (2 * wc + ni))) +
                      (B_BIASED ? U_BLO : 0);
    }
  }
  {
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
}

// One 64-row half of a wave's output through its private LDS image: acc rows
// r0..r0+3, to C rows crow.., as in wgrad_gemm_kernel's epilogue.
template <int ROWS>
DEVINL void wg_store_half(float* ep, const f32x4 (&acc)[ROWS][4], int r0,
                          bf16_t* __restrict__ C, long crow, long ccol, long K,
                          int lane, int accumulate) {
  const int fr = lane & 15, fq = lane >> 4;
  const int orow = lane >> 3, ocol = (lane & 7) * 8;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        ep[(mi * 16 + fq * 4 + j) * EPI_LD + ni * 16 + fr] =
            acc[r0 + mi][ni][j];
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int row = it * 8 + orow;
    const float* src = ep + row * EPI_LD + ocol;
    const f32x4 v0 = *(const f32x4*)src;
    const f32x4 v1 = *(const f32x4*)(src + 4);
    float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    bf16_t* dst = C + (crow + row) * K + ccol;
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

// A full 256 x 256 tile by schedule VARIANT (0: wgrad_tile, 1: wgrad_tile_v1).
template <int VARIANT>
DEVINL void wgrad_full_block(char* smem, const bf16_t* __restrict__ dy,
                             const bf16_t* __restrict__ x,
                             bf16_t* __restrict__ C, int T, int N, int K,
                             int accumulate, unsigned tn, unsigned tk) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 2, wc = wid & 3;
  const long n0 = (long)tn * WG_TILE, k0 = (long)tk * WG_TILE;
  WgCtx c;
  wg_setup<VARIANT != 0>(c, smem, tid, wr, wc, dy, x, n0, k0, T, N, K);

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

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
  if constexpr (VARIANT == 0) {
    for (; t + 1 < T; t += 2) {
      wgrad_tile<0>(c, t, acc);
      wgrad_tile<1>(c, t + 1, acc);
    }
    if (t < T) wgrad_tile<0>(c, t, acc);
  } else {
    bf16x8v a[4][2], b0[2][2], b1[2][2];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) read_a1<U_ALO, 0>(c, a, mi, 0);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) read_b1<U_BLO, 0>(c, b0, ni, s);
    for (; t + 1 < T; t += 2) {
      wgrad_tile_v1<0>(c, t, acc, a, b0, b1);
      wgrad_tile_v1<1>(c, t + 1, acc, a, b0, b1);
    }
    if (t < T) wgrad_tile_v1<0>(c, t, acc, a, b0, b1);
  }

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  float* ep = (float*)smem + wid * 64 * EPI_LD;
  const int ocol = (lane & 7) * 8;
  const long ccol = k0 + (ocol >> 5) * 128 + wc * 32 + (ocol & 31);
#pragma unroll
  for (int h = 0; h < 2; ++h)
    wg_store_half(ep, acc, h * 4, C, n0 + h * 128 + wr * 64, ccol, (long)K,
                  lane, accumulate);
}

// Half block: rows 128 hb .. 128 hb + 127 of a tile, all 256 columns. Wave
// (wr, wc) owns rows 64 wr.. of the one A unit and columns 32 wc.. of both B
// units, so every 16 x 16 accumulator sees the fragments, the MFMAs and the
// order a full block gives it. Units A, B_lo, B_hi, two buffers each, at the
// full block's U_ALO, U_BLO, U_BHI. Two phases per tile; the fragments of
// tile t + 1 are read from buffer b ^ 1 during tile t into a second
// register set (a, b1) or the idle one (b0).
template <int BUF>
DEVINL void wgrad_half_tile(const WgCtx& c, int t,
                            f32x4 (&acc)[4][4], bf16x8v (&a)[2][4][2],
                            bf16x8v (&b0)[2][2], bf16x8v (&b1)[2][2][2]) {
  const long t2 = min(t + 2, c.last), t3 = min(t + 3, c.last);
  const char* x2 = c.x0 + t2 * c.x_step;
  const char* dy3 = c.dy0 + t3 * c.dy_step;

  // phase 0: C[h][lo]; reads all of A[BUF ^ 1]
  phase_open();
  stage_unit<U_BLO, BUF>(c, x2, c.vx);
  stage_unit<U_BHI, BUF>(c, x2 + 256, c.vx);
  mma_open();
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    mma_pair<0, 0>(acc, a[BUF], b0, 0, mi);
    read_a1<U_ALO, BUF ^ 1>(c, a[BUF ^ 1], mi, 0);
    read_a1<U_ALO, BUF ^ 1>(c, a[BUF ^ 1], mi, 1);
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) mma_pair<0, 0>(acc, a[BUF], b0, 1, mi);
  mma_close();
  wait_lds_reads();                                   // A[BUF ^ 1] is free
  asm volatile("s_waitcnt vmcnt(6)" ::: "memory");    // B_lo, B_hi[BUF ^ 1]
  __builtin_amdgcn_sched_barrier(0);

  // phase 1: C[h][hi]; reads B_lo and B_hi[BUF ^ 1]
  phase_open();
  stage_unit<U_ALO, BUF ^ 1>(c, dy3, c.vdy);
  mma_open();
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    mma_pair<0, 1>(acc, a[BUF], b1[BUF], 0, mi);
    read_b1<U_BLO, BUF ^ 1>(c, b0, mi & 1, mi >> 1);
    read_b1<U_BHI, BUF ^ 1>(c, b1[BUF ^ 1], mi & 1, mi >> 1);
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) mma_pair<0, 1>(acc, a[BUF], b1[BUF], 1, mi);
  mma_close();
  wait_lds_reads();                                   // B[BUF ^ 1] is free
  asm volatile("s_waitcnt vmcnt(6)" ::: "memory");    // A[BUF] of tile t + 2
  __builtin_amdgcn_sched_barrier(0);
}

DEVINL void wgrad_half_block(char* smem, const bf16_t* __restrict__ dy,
                             const bf16_t* __restrict__ x,
                             bf16_t* __restrict__ C, int T, int N, int K,
                             int accumulate, unsigned tn, unsigned tk,
                             int hb) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 2, wc = wid & 3;
  const long n0 = (long)tn * WG_TILE + hb * 128, k0 = (long)tk * WG_TILE;
  WgCtx c;
  wg_setup<true>(c, smem, tid, wr, wc, dy, x, n0, k0, T, N, K);

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8v a[2][4][2], b0[2][2], b1[2][2][2];

  // prologue: tiles 0 and 1 whole, tile 0 into registers, then A of tile 2
  {
    const long t1 = min(1, c.last), t2 = min(2, c.last);
    const char* dy1 = c.dy0 + t1 * c.dy_step;
    const char* x1 = c.x0 + t1 * c.x_step;
    stage_unit<U_ALO, 0>(c, c.dy0, c.vdy);
    stage_unit<U_BLO, 0>(c, c.x0, c.vx);
    stage_unit<U_BHI, 0>(c, c.x0 + 256, c.vx);
    stage_unit<U_ALO, 1>(c, dy1, c.vdy);
    stage_unit<U_BLO, 1>(c, x1, c.vx);
    stage_unit<U_BHI, 1>(c, x1 + 256, c.vx);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    wg_barrier();
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      read_a1<U_ALO, 0>(c, a[0], mi, 0);
      read_a1<U_ALO, 0>(c, a[0], mi, 1);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        read_b1<U_BLO, 0>(c, b0, ni, s);
        read_b1<U_BHI, 0>(c, b1[0], ni, s);
      }
    wait_lds_reads();
    wg_barrier();
    stage_unit<U_ALO, 0>(c, c.dy0 + t2 * c.dy_step, c.vdy);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");    // A[1] of tile 1
    __builtin_amdgcn_sched_barrier(0);
  }

  int t = 0;
  for (; t + 1 < T; t += 2) {
    wgrad_half_tile<0>(c, t, acc, a, b0, b1);
    wgrad_half_tile<1>(c, t + 1, acc, a, b0, b1);
  }
  if (t < T) wgrad_half_tile<0>(c, t, acc, a, b0, b1);

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  float* ep = (float*)smem + wid * 64 * EPI_LD;
  const int ocol = (lane & 7) * 8;
  const long ccol = k0 + (ocol >> 5) * 128 + wc * 32 + (ocol & 31);
  wg_store_half(ep, acc, 0, C, n0 + wr * 64, ccol, (long)K, lane, accumulate);
}

// Blocks 0..nfull-1: full tiles 0..nfull-1 of the raster, XCD remap over
// nfull. Blocks nfull..: the halves of tiles nfull.. . Blocks l and l + 8 of
// a run of 16 are the two halves of one tile, so that under round-robin
// dispatch both read their x slabs through one XCD's L2; a last run shorter
// than 16 pairs neighbours.
template <int VARIANT>
__global__ __launch_bounds__(WG_NTH, 2) void wgrad_gemm_split_kernel(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
    bf16_t* __restrict__ C, int T, int N, int K, int accumulate, int group,
    unsigned nfull) {
  __shared__ __attribute__((aligned(1024))) char smem[WG_LDS_BYTES];
  const unsigned TN = N / WG_TILE, TK = K / WG_TILE;
  const unsigned l = blockIdx.x;
  unsigned tn, tk;
  if (l >= nfull) {
    const unsigned lh = l - nfull, nh = gridDim.x - nfull;
    const unsigned whole = nh & ~15u;
    unsigned j, hb;
    if (lh < whole) {
      j = (lh >> 4) * 8 + (lh & 7);
      hb = (lh >> 3) & 1;
    } else {
      j = (whole >> 1) + ((lh - whole) >> 1);
      hb = lh & 1;
    }
    wg_raster(nfull + j, TN, TK, group, tn, tk);
    wgrad_half_block(smem, dy, x, C, T, N, K, accumulate, tn, tk, (int)hb);
    return;
  }
  const unsigned q = nfull >> 3, r = nfull & 7, xcd = l & 7;
  const unsigned w =
      (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (l >> 3);
  wg_raster(w, TN, TK, group, tn, tk);
  wgrad_full_block<VARIANT>(smem, dy, x, C, T, N, K, accumulate, tn, tk);
}

}  // namespace

// Trailing tiles to compute as half blocks: with r = tiles % cus left for the
// last round, r when they fill at most the round as 2r halves, else 0.
extern "C" long tok_wgrad_split(long tiles, long cus) {
  if (tiles < 0 || cus < 1) return 0;
  const long r = tiles % cus;
  return (r > 0 && 2 * r <= cus) ? r : 0;
}

// Compute units of the current device, asked once per device.
extern "C" hipError_t tok_wgrad_cus(int* cus) {
  static int cached[64] = {0};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
  if (cached[dev] == 0) {
    int n = 0;
    e = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    if (n < 1) return hipErrorInvalidDevice;
    cached[dev] = n;
  }
  *cus = cached[dev];
  return hipSuccess;
}

extern "C" int tok_wgrad_default_variant() { return WG_DEFAULT_VARIANT; }

// C[N,K] = (accumulate ? C : 0) + dy[M,N]^T x[M,K], all bf16 row-major and
// 16-byte aligned; M % 64 == 0, N % 256 == 0, K % 256 == 0. `group` is the
// raster's band height in dy slabs (>= 1). `variant`: 0 the two-barrier
// schedule, 1 reads under the MFMAs, < 0 the default. `split`: trailing
// tiles computed as two half blocks each, < 0 for tok_wgrad_split's rule.
// Every choice gives the same bits. Launches on `stream` only: no
// allocation, copy or sync, so the call can be captured.
extern "C" hipError_t tok_wgrad_gemm(const void* dy, const void* x, void* c,
                                     long M, long N, long K, int accumulate,
                                     int group, int variant, long split,
                                     hipStream_t stream) {
  if (M < WG_BK || M % WG_BK || N < WG_TILE || N % WG_TILE || K < WG_TILE ||
      K % WG_TILE || group < 1)
    return hipErrorInvalidValue;
  // lane offsets of the DMA are 32-bit: 64 rows of the wider operand
  if (64 * (N > K ? N : K) * 2 >= (1L << 31) || M / WG_BK >= (1L << 30))
    return hipErrorInvalidValue;
  const long tiles = (N / WG_TILE) * (K / WG_TILE);
  if (tiles >= (1L << 30)) return hipErrorInvalidValue;
  if (group > N / WG_TILE) group = (int)(N / WG_TILE);   // one band at most
  if (variant < 0) variant = WG_DEFAULT_VARIANT;
  if (variant > 1 || split > tiles) return hipErrorInvalidValue;
  if (split < 0) {
    int cus = 0;
    const hipError_t e = tok_wgrad_cus(&cus);
    if (e != hipSuccess) return e;
    split = tok_wgrad_split(tiles, cus);
  }
  const unsigned nfull = (unsigned)(tiles - split);
  const dim3 grid((unsigned)(tiles + split));
  if (variant == 0 && split == 0)
    wgrad_gemm_kernel<<<grid, WG_NTH, 0, stream>>>(
        (const bf16_t*)dy, (const bf16_t*)x, (bf16_t*)c, (int)(M / WG_BK),
        (int)N, (int)K, accumulate, group);
  else if (variant == 0)
    wgrad_gemm_split_kernel<0><<<grid, WG_NTH, 0, stream>>>(
        (const bf16_t*)dy, (const bf16_t*)x, (bf16_t*)c, (int)(M / WG_BK),
        (int)N, (int)K, accumulate, group, nfull);
  else
    wgrad_gemm_split_kernel<1><<<grid, WG_NTH, 0, stream>>>(
        (const bf16_t*)dy, (const bf16_t*)x, (bf16_t*)c, (int)(M / WG_BK),
        (int)N, (int)K, accumulate, group, nfull);
  return hipGetLastError();
}
