// lstm_persist.hip — persistent, XCD-local LSTM sequence kernels (fast path for H in {128, 256, 320, 512}, 8 or 4
// rows per XCD).
//
// Why: with one launch per time step every step pays a kernel boundary (~1.7 us) plus a cold start — L2 does not
// survive the boundary, so the 8 MB of recurrent weights are re-streamed from Infinity Cache 1 400 times per
// direction and pass.  Here ONE launch runs the whole sequence:
//   * the 8 XCDs each take one (direction, 8-batch-row group); the XCD's 32 CUs each own 16 hidden units
//     (64 gate-interleaved rows of W_hh) and keep that 128 KB slice in REGISTERS for all T steps
//     (8 waves x 64 VGPRs: wave w holds the K range [64w, 64w+64));
//   * per step only h_t of the group (8 rows x 512 units = 16 KB) is exchanged, inside the XCD, as fp32 words whose
//     mantissa LSB is a validity tag, written with plain workgroup-scope stores (they stay in the XCD's L2) and read
//     with 16-byte sc1 buffer loads that bypass L1.  The data is the flag: no fences, no separate counters, and
//     correctness does not depend on which CU/XCD a workgroup landed on — only the speed does.  (The first version
//     used 8-byte {tag = step+1, value} granules and agent-scope atomics: 2.35 us per step against 2.05.)
//   * the gate product runs on v_mfma_f32_4x4x1_16b_f32: its 16 blocks are this CU's 16 units, A = the 4 gates
//     of a unit (one W register per k), B = 4 batch rows of h; K accumulates over instructions, so the 4 gate
//     pre-activations of a (unit, row) land in one lane and the pointwise update needs no shuffles.  The 8
//     waves' K-partials are summed through LDS.
// Roles come from HW_REG_XCC_ID + a per-XCC ticket.  Every spin is bounded; on a timeout or an unexpected
// placement the kernel raises an abort word, poisons its outputs with NaN and drains — the host falls back to
// the per-step kernels.  1 workgroup per CU is enforced by the LDS request, so 256 workgroups are co-resident.
#include <cstdlib>
#include <type_traits>
#include "persist.h"
// measurement only: shader-clock stamps of workgroup (group 0, slice 0), time steps 8..15, into ctrl[16..]
#ifdef ASR_LP_TRACE
#define LP_MARK(k) do { if ((tid == 0 || tid == 448) && g == 0 && slice == 0 && s >= 8 && s < 16) \
    ((unsigned long long*)(a.ctrl + 16))[(tid ? 128 : 0) + (s - 8) * 16 + (k)] = clock64(); } while (0)
#elif defined(ASR_LP_TRACE2)
// per-CU imbalance probe: (top of step, tile gathered) of wave 0 of every slice of group 0, steps 8..15
#define LP_MARK(k) do { if (tid == 0 && g == 0 && s >= 8 && s < 16 && ((k) == 0 || (k) == 1)) \
    ((unsigned long long*)a.ctrl)[(slice * 8 + (s - 8)) * 2 + (k)] = clock64(); } while (0)
#else
#define LP_MARK(k) do {} while (0)
#endif

namespace {

constexpr int ASR_LSTM_TOUCH = 1;
constexpr int ASR_LSTM_TOUCH_DIST = 3;
// waves whose first poll attempt requests the whole tile (16-byte loads: 8 per lane); with the 8-byte loads only the
// pointwise waves (2) paid off: 3.85 (2) -> 3.78 (4) -> 3.62 (8) us per step
constexpr int ASR_LSTM_BWD_FULL_WAVES = 8;
constexpr int ASR_LSTM_FULL_WAVES = 2;            // waves 0..1 hold the pointwise threads (PUC*PRG <= 128)
constexpr int ASR_ABORT_PERIOD_MASK = 15;         // the abort word is polled when (step & mask) == 0; 0 = every step (first version)
// forward (split-bf16) kernel: groups of at least this many rows spin on one quad per lane before requesting the tile (99 = never)
constexpr int ASR_POLL_SENTINEL_ROWS = 16;
// s_sleep between two poll attempts.  0 / 1 / 2 / 4 / 8 measured 1.72 / 1.75 / 1.75 / 1.84 / 1.93 us per forward step and
// 1.82 / 1.82 / 1.81 / 1.82 / 2.19 backward (H = 512, 8 rows): failed polls do not clog the L2 (DESIGN_HISTORY, round 4)
constexpr int POLL_SLEEP = 1;

// Hidden sizes: H % 32 == 0 and H <= 512 (a CU's H/32 units must fit the 16 MFMA blocks; instantiated for 128,
// 256, 320, 512).  Blocks / lanes beyond a smaller H idle.
constexpr int PW = 8;            // waves per workgroup
constexpr int PNT = PW * 64;     // 512 threads
constexpr int PRG = 8;           // batch rows per XCD group

// Row of (time tt, this thread's batch row) in gates / y / c / dy.  A macro over the kernel's locals (B, prow, pbase, pext) and
// its template parameter PACKED; see PersistArgs and the note in lstm_persist_bwd_rs_kernel.
#define ROW_AT(tt_) (PACKED ? (int64_t)(pbase + ((tt_) < pext ? (tt_) : pext - 1)) : ((int64_t)(tt_) * B + prow))

struct PersistArgs {
  int T, B, nb, ndir;
  float* gates;         // [T][B][ndir][4H]
  const float* w;       // fwd: w_hh [ndir][4H][H];  bwd: w_hhT [ndir][H][4H]
  const float* w_il;    // bwd, exchanged-partials kernel only: w_hh in the forward layout instead of w (saves the caller a transpose), or NULL
  const int32_t* lens;
  float* y;             // fwd: out y;  bwd: unused
  float* c;             // [T][B][ndir*H]
  const float* dy;      // bwd
  const float* yfwd;    // bwd: forward hidden states [T][B][ndir*H] (partner of dG in dW_hh), or NULL
  float* dw;            // bwd: dW_hh [ndir][4H][H] gate-interleaved, accumulated with atomics, or NULL
  float* db;            // bwd: bias gradient [ndir][4H] gate-interleaved (sum of dG over time and rows), or NULL
  u64* xch;             // fwd: [2][8][PRG][H] granules;  bwd: [2][8][PRG][4H]
  unsigned* ctrl;       // [0..7] tickets per XCC, [8] abort, [9] error code
  // Row addressing of gates / y / c / dy.  NULL: time-major, row (t, b) = t * B + b, every row has all T times.  Otherwise
  // PACKED rows (include/asr_hip.h): batch row b owns rows rowbase[b] .. rowbase[b] + rowext[b] - 1, time t at rowbase[b] + t;
  // lens[b] < rowext[b], the rows lens[b] .. rowext[b] - 1 are written as padding (zeros), times >= rowext[b] do not exist
  // (nothing is stored; loads are clamped to the last row of the block, their values are dead).
  const int32_t* rowbase;
  const int32_t* rowext;
};

// ---------------------------------------------------------------------------------------------------- forward
// NR = batch rows per group actually used (8, or 4 for small batches: half the MFMA work and half the gather per step;
// the exchange and LDS layouts keep their 8-row shape, rows NR..7 are simply never touched).
template <int PH, int NR, bool PACKED = false>
__global__ __launch_bounds__(PNT) void lstm_persist_fwd_kernel(PersistArgs a) {
  static_assert(NR == 4 || NR == PRG, "rows per group");
  constexpr int PKW = PH / PW;     // K columns per wave
  constexpr int PUC = PH / 32;     // hidden units per CU (<= 16 MFMA blocks)
  // this wave's K range of h_{t-1}; rows padded by 4 floats so the 4 rows a ds_read_b128 touches (the MFMA blocks
  // broadcast) fall on different bank slots
  __shared__ __attribute__((aligned(16))) float hs[PW][PRG][PKW + 4];
  __shared__ __attribute__((aligned(16))) float part[2][PW][64][8];      // K-partials, double buffered (32 KB)
  __shared__ int role[2];
  extern __shared__ float occupancy_pad[];                                // forces one workgroup per CU
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int g, slice;
  take_role(a.ctrl, role, g, slice);
  if (slice < 0) return;
  const int T = a.T, B = a.B, ndir = a.ndir;
  const int d = ndir == 2 ? (g & 1) : 0;
  const int rowgroup = ndir == 2 ? (g >> 1) : g;
  const int r0 = rowgroup * NR;
  if (r0 >= a.nb) return;                      // this group has no rows (nobody waits for it)
  const int64_t ldy = (int64_t)ndir * PH;
  // recurrent weights of this CU -> registers: lane owns gate-interleaved row 64*slice+lane, wave owns 64 k's
  float wreg[PKW];
  {
    const int wrow = lane < 4 * PUC ? lane : 0;       // lanes beyond this CU's 4*PUC gate rows idle (results unused)
    const float* wr = a.w + ((int64_t)d * 4 * PH + 4 * PUC * slice + wrow) * PH + wave * PKW;
#pragma unroll
    for (int k4 = 0; k4 < PKW / 4; ++k4) {
      const float4 v = *reinterpret_cast<const float4*>(wr + 4 * k4);
      wreg[4 * k4] = v.x; wreg[4 * k4 + 1] = v.y; wreg[4 * k4 + 2] = v.z; wreg[4 * k4 + 3] = v.w;
    }
  }
  // pointwise ownership: thread (pu, pj) for tid < 128 -> unit 16*slice+pu, row r0+pj
  const int pu = tid >> 3, pj = tid & 7;
  const bool pw_thread = tid < PUC * PRG && pj < NR;
  const int prow = r0 + pj;
  const bool prow_ok = pw_thread && prow < a.nb;
  const int punit = PUC * slice + pu;
  const int plen = prow_ok ? a.lens[prow] : 0;
  // row of (time, this thread's batch row): see PersistArgs and the note in lstm_persist_bwd_rs_kernel
  const int pbase = (PACKED && prow_ok) ? a.rowbase[prow] : 0;
  const int pext = PACKED ? (prow_ok ? a.rowext[prow] : 1) : a.T;
  float c_prev = 0.f;
  u64* xch_g = a.xch + (int64_t)g * PRG * PH;          // + parity * 8*PRG*PH
  float* xw_g = reinterpret_cast<float*>(a.xch) + (int64_t)g * 2 * PH * PRG;   // word protocol: [parity][unit][row]
  const int64_t par_stride = (int64_t)8 * PRG * PH;
  typedef unsigned u4v __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(a.xch, 0, 0x7ffffff0, 0x00020000);
  bool aborted = false;
  // The x-projection rows are fetched TWO steps ahead: they are HBM first-touch loads (~2 us under load, about one
  // forward step), vmcnt retires in order, and the row is consumed at the top of its step -- one step of distance
  // left the pointwise waves waiting ~1 300 cycles there (tools/lstm_trace.py).
  auto gx_ptr = [&](int sn) {
    const int tt = d == 0 ? sn : T - 1 - sn;
    return reinterpret_cast<const float4*>(a.gates + (ROW_AT(tt) * ndir + d) * 4 * PH + punit * 4);
  };
  float4 gx_n1 = make_float4(0.f, 0.f, 0.f, 0.f), gx_n2 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (prow_ok) {
    gx_n1 = *gx_ptr(0);
    if (T > 1) gx_n2 = *gx_ptr(1);
  }
  // Bulk outputs of a step (gates, c, y) are stored AFTER the next step's gather: vmcnt counts stores too and retires
  // in order, so a store issued just before the poll keeps the poll's loads waiting for its write acknowledgement
  // (~1 000+ cycles on the serial chain of the pointwise waves).  Deferred, the acknowledgements overlap the MFMAs.
  float4 st_g = make_float4(0.f, 0.f, 0.f, 0.f);
  float st_c = 0.f, st_y = 0.f;
  float4* st_gp = nullptr;
  int64_t st_so = 0;
  for (int s = 0; s < T; ++s) {
    const int t = d == 0 ? s : T - 1 - s;
    // abort word sampled at the top of the step: consumed by the pointwise phase long after it has arrived (an L2
    // round trip issued there would sit on the serial chain of every time step)
    LP_MARK(0);
    const unsigned abort_seen = pw_thread ? flag_load(a.ctrl + 8) : 0u;
    const float4 gx = gx_n1;
    gx_n1 = gx_n2;
    float4* gp = nullptr;
    if (prow_ok) gp = reinterpret_cast<float4*>(a.gates + (ROW_AT(t) * ndir + d) * 4 * PH + punit * 4);
    f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (s > 0) {
      // Single-stage hand-off, 16-byte reads: h_{t-1} travels as LSB-tagged fp32 words laid out [unit][row], so the rows
      // of a lane's unit are contiguous and one sc1 buffer load (two for 8 rows) is data and flag at once: no sentinel
      // round trip, and a quarter of the load instructions of the 8-byte granule protocol.
      const bool gl = lane < PKW;
      const unsigned boff = (unsigned)((xw_g - reinterpret_cast<float*>(a.xch)) + ((s - 1) & 1) * (PH * PRG) +
                                       (wave * PKW + (gl ? lane : 0)) * PRG) * 4u;
      const unsigned tb = tag_bit_of_step(s - 1);
      u4v gw[NR / 4];
      unsigned spins = 0;
      while (true) {
#pragma unroll
        for (int j = 0; j < NR / 4; ++j) gw[j] = __builtin_amdgcn_raw_buffer_load_b128(xrs, boff + 16u * j, 0, 16);
        unsigned bits = 1u;
#pragma unroll
        for (int j = 0; j < NR / 4; ++j) bits &= ~(gw[j].x ^ tb) & ~(gw[j].y ^ tb) & ~(gw[j].z ^ tb) & ~(gw[j].w ^ tb);
        LP_MARK(7);
        if (__all(!gl || (bits & 1u))) break;
        if (++spins > SPIN_LIMIT || ((spins & 63u) == 0u && flag_load(a.ctrl + 8) != 0u)) {
          if (lane == 0) raise_abort(a.ctrl, 1u);
          aborted = true;
          break;
        }
        __builtin_amdgcn_s_sleep(POLL_SLEEP);
      }
      LP_MARK(1);
#ifdef ASR_LP_TRACE
      if (tid == 0 && g == 0 && slice == 0 && s >= 8 && s < 16) ((unsigned long long*)(a.ctrl + 16))[(s - 8) * 16 + 8] = spins;
#endif
#pragma unroll
      for (int j = 0; j < NR / 4; ++j)
        if (gl) {
          hs[wave][4 * j][lane] = __uint_as_float(gw[j].x); hs[wave][4 * j + 1][lane] = __uint_as_float(gw[j].y);
          hs[wave][4 * j + 2][lane] = __uint_as_float(gw[j].z); hs[wave][4 * j + 3][lane] = __uint_as_float(gw[j].w);
        }
      if (st_gp) {                    // previous step's outputs (see above)
        *st_gp = st_g;
        a.c[st_so] = st_c;
        a.y[st_so] = st_y;
        st_gp = nullptr;
      }
      if (prow_ok && s + 2 < T) gx_n2 = *gx_ptr(s + 2);     // in flight for two steps
      // (wave-private LDS region: program order within the wave is enough)
      const int j = lane & 3;
#pragma unroll
      for (int k4 = 0; k4 < PKW / 4; ++k4) {
        // consecutive MFMAs alternate between two accumulators (a dependent chain on one would stall the pipe): rows
        // 0-3 / 4-7 with 8 rows per group, even / odd k (summed below) with 4
        const float4 b0 = *reinterpret_cast<const float4*>(&hs[wave][j][4 * k4]);
        if (NR > 4) {
          const float4 b1 = *reinterpret_cast<const float4*>(&hs[wave][4 + j][4 * k4]);
          acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * k4], b0.x, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * k4], b1.x, acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * k4 + 1], b0.y, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * k4 + 1], b1.y, acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * k4 + 2], b0.z, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * k4 + 2], b1.z, acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * k4 + 3], b0.w, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * k4 + 3], b1.w, acc1, 0, 0, 0);
        } else {
          acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * k4], b0.x, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * k4 + 1], b0.y, acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * k4 + 2], b0.z, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * k4 + 3], b0.w, acc1, 0, 0, 0);
        }
      }
      if (NR <= 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc0[i] += acc1[i];
      }
    }
    if (s == 0 && prow_ok && T > 2) gx_n2 = *gx_ptr(2);
    LP_MARK(2);
    float* pp = &part[s & 1][wave][lane][0];
    *reinterpret_cast<float4*>(pp) = make_float4(acc0[0], acc0[1], acc0[2], acc0[3]);
    if (NR > 4) *reinterpret_cast<float4*>(pp + 4) = make_float4(acc1[0], acc1[1], acc1[2], acc1[3]);
    LP_MARK(3);
    __syncthreads();
    LP_MARK(4);
    if (pw_thread) {
      // lane holding (unit pu, row pj): 4*pu + (pj&3); registers 4*(pj>>2) + gate
      float pre[4] = {gx.x, gx.y, gx.z, gx.w};
      const int pl = 4 * pu + (pj & 3), pr = 4 * (pj >> 2);
#pragma unroll
      for (int w2 = 0; w2 < PW; ++w2) {          // one 16-byte read per wave (the 8 threads of a unit read 128 contiguous bytes)
        const float4 v = *reinterpret_cast<const float4*>(&part[s & 1][w2][pl][pr]);
        pre[0] += v.x; pre[1] += v.y; pre[2] += v.z; pre[3] += v.w;
      }
      const float gi = asr_fast_sigmoid(pre[0]), gf = asr_fast_sigmoid(pre[1]);
      const float gg = asr_fast_tanh(pre[2]), go = asr_fast_sigmoid(pre[3]);
      float cn = gf * c_prev + gi * gg;
      float hn = go * asr_fast_tanh(cn);
      if (t >= plen) { cn = 0.f; hn = 0.f; }
      if (aborted || abort_seen != 0u) hn = __builtin_nanf("");
      c_prev = cn;
      LP_MARK(5);
      word_store(xw_g + (s & 1) * (PH * PRG) + (int64_t)punit * PRG + pj, hn, tag_bit_of_step(s));       // hand-off first
#ifdef ASR_LP_TRACE3   /* visibility probe: global 100 MHz clock at the publish of (slice 28, row 7, its first unit) ... */
      if (g == 0 && slice == 28 && tid == 7 && s < 64) ((unsigned long long*)a.ctrl)[16 + 2 * s] = wall_clock64();
#endif
      if (prow_ok && (!PACKED || t < pext)) {
        st_g = make_float4(gi, gf, gg, go); st_c = cn; st_y = hn;
        st_gp = gp;
        st_so = ROW_AT(t) * ldy + d * PH + punit;
      }
      LP_MARK(6);
    }
  }
  if (st_gp) {
    *st_gp = st_g;
    a.c[st_so] = st_c;
    a.y[st_so] = st_y;
  }
  // packed rows: the block's padding rows behind the T steps that were run (times T .. rowext - 1; PersistArgs)
  if constexpr (PACKED) if (prow_ok) {
    for (int tt = T; tt < pext; ++tt) {
      const int64_t so = ROW_AT(tt) * ldy + d * PH + punit;
      a.c[so] = 0.f;
      a.y[so] = 0.f;
    }
  }
}

// ------------------------------------------------------------------------------- forward, split-bf16 products
// Same organisation as lstm_persist_fwd_kernel (roles, exchange of LSB-tagged words laid out [unit][row], pointwise
// ownership, deferred stores); the gate product runs on v_mfma_f32_16x16x32_bf16 with both operands split into two
// bf16 terms, x = hi + lo (hi = the upper 16 bits of the fp32 word, lo = the upper 16 bits of x - hi: 16 significand
// bits in all), and three products hi*hi + hi*lo + lo*hi accumulated in fp32.  The dropped lo*lo term and the
// truncation are <= 2^-15 relative per operand pair (fp32 itself: 2^-24) - two orders of magnitude inside the 1e-3
// parity gate, measured in tests/test_hip_parity.py::test_lstm_persistent_path - while the bf16 pipe runs 16x the rate
// of the fp32 MFMA: the product leaves the serial chain of a time step (1 024 -> 384 MFMA cycles per wave at H = 512).
//   A = W_hh: M tile mt = gate rows 16 mt .. 16 mt + 15 of this CU (4 units x 4 gates), lane l holds row l & 15,
//       k = 32 ks + 8 (l >> 4) + j of the wave's K range, j = 0..7, as bf16x8: registers for the whole sequence;
//   B = h_{t-1}: lane l holds batch row l & 15 (rows >= 8 alias row l & 7, their columns of D are never read),
//       the same 8 k's, read from the wave's LDS tile as one 16-byte load per term;
//   D: lane l holds gate rows 16 mt + 4 (l >> 4) + i = the four gates of unit 4 mt + (l >> 4) for batch row l & 15:
//       exactly the float4 the pointwise thread of (unit, row) sums over the 8 waves.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned bf3_hi(float v) { return __float_as_uint(v) >> 16; }
__device__ __forceinline__ unsigned bf3_lo(float v) {
  return __float_as_uint(v - __uint_as_float(__float_as_uint(v) & 0xffff0000u)) >> 16;
}
__device__ __forceinline__ void bf3_split8(const float (&v)[8], u32x4& hi, u32x4& lo) {
  hi = (u32x4){bf3_hi(v[0]) | (bf3_hi(v[1]) << 16), bf3_hi(v[2]) | (bf3_hi(v[3]) << 16),
               bf3_hi(v[4]) | (bf3_hi(v[5]) << 16), bf3_hi(v[6]) | (bf3_hi(v[7]) << 16)};
  lo = (u32x4){bf3_lo(v[0]) | (bf3_lo(v[1]) << 16), bf3_lo(v[2]) | (bf3_lo(v[3]) << 16),
               bf3_lo(v[4]) | (bf3_lo(v[5]) << 16), bf3_lo(v[6]) | (bf3_lo(v[7]) << 16)};
}
// NT-term split of one value / eight values.  NT = 2: hi + lo as above (truncating; the "bf16x3" arithmetic).  NT = 3
// ("bf16x6", the default): a = bf16(x), b = bf16(x - a), c = x - a - b, every conversion rounded to nearest; both
// differences are exact in fp32 and c has at most 8 significand bits, so a + b + c == x exactly (see gemm.hip).
typedef __bf16 lbf16x2 __attribute__((ext_vector_type(2)));
template <int NT>
__device__ __forceinline__ void bfn_split1(float v, unsigned (&t)[NT]) {          // 16-bit patterns, most significant first
  if constexpr (NT == 2) {
    t[0] = bf3_hi(v);
    t[1] = bf3_lo(v);
  } else {
    const lbf16x2 pa = {(__bf16)v, (__bf16)0.f};
    const unsigned ua = __builtin_bit_cast(unsigned, pa) & 0xffffu;
    const float r = v - __uint_as_float(ua << 16);
    const lbf16x2 pb = {(__bf16)r, (__bf16)0.f};
    const unsigned ub = __builtin_bit_cast(unsigned, pb) & 0xffffu;
    const float q = r - __uint_as_float(ub << 16);
    t[0] = ua; t[1] = ub; t[2] = __float_as_uint(q) >> 16;
  }
}
template <int NT>
__device__ __forceinline__ void bfn_split2(float x, float y, unsigned (&t)[NT]) {  // t[k] = {term_k(x), term_k(y)}
  if constexpr (NT == 2) {
    t[0] = bf3_hi(x) | (bf3_hi(y) << 16);
    t[1] = bf3_lo(x) | (bf3_lo(y) << 16);
  } else {
    const lbf16x2 pa = {(__bf16)x, (__bf16)y};
    const unsigned ua = __builtin_bit_cast(unsigned, pa);
    const float rx = x - __uint_as_float(ua << 16), ry = y - __uint_as_float(ua & 0xffff0000u);
    const lbf16x2 pb = {(__bf16)rx, (__bf16)ry};
    const unsigned ub = __builtin_bit_cast(unsigned, pb);
    const float sx = rx - __uint_as_float(ub << 16), sy = ry - __uint_as_float(ub & 0xffff0000u);
    t[0] = ua; t[1] = ub;
    t[2] = __builtin_amdgcn_perm(__float_as_uint(sy), __float_as_uint(sx), 0x07060302u);
  }
}
template <int NT>
__device__ __forceinline__ void bfn_split8(const float (&v)[8], u32x4 (&t)[NT]) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    unsigned q[NT];
    bfn_split2<NT>(v[2 * p], v[2 * p + 1], q);
#pragma unroll
    for (int k = 0; k < NT; ++k) t[k][p] = q[k];
  }
}
// Three-term products on a 16-column MFMA whose batch side has only 8 rows: the idle columns 8..15 carry a second term of
// the batch-side operand, so that the six products of a (weight tile, k-step) take FOUR instructions instead of six:
//   B1 = [a | b] (columns 0..7 | 8..15),  B2 = [c | 0]
//   D += Wa B1 + Wb B1 + Wc B1 + Wa B2   ->   columns 0..7: aa + ba + ca + ac,   columns 8..15: ab + bb + cb
// (cb' is one of the three dropped 2^-24 terms; it comes for free and is kept).  The two halves are added once, after the
// k loop, with one row_ror:8 DPP add per accumulator element (done on scalar copies: applied to the elements of the MFMA
// accumulator vector in place, hipcc 7.2 paired the rotations with the wrong elements).
__device__ __forceinline__ void fold_halves(f32x4& acc) {
  float v[4] = {acc[0], acc[1], acc[2], acc[3]};
#pragma unroll
  for (int i = 0; i < 4; ++i)
    v[i] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v[i]), 0x128, 0xf, 0xf, true));
  acc = (f32x4){v[0], v[1], v[2], v[3]};
}
__device__ __forceinline__ f32x4 bf3_mfma(const u32x4& a, const u32x4& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// RG = rows of a group in the exchange / LDS layouts: 8 (NR = 8 or 4 active rows), or 16 (NR = 16: batches of >= 64 rows run
// 16 rows per XCD group - the MFMA's 16 batch columns all carry rows, six products per tile and k-step instead of the
// folded four, twice the gather - so that two 32-row blocks share one traversal of the chain).
template <int PH, int NR, int NT, int RG = PRG, bool PACKED = false, bool FAULT = false>
__global__ __launch_bounds__(PNT) void lstm_persist_fwd_bf3_kernel(PersistArgs a) {
  static_assert((RG == PRG && (NR == 4 || NR == PRG)) || (RG == 16 && NR == 16), "rows per group");
  constexpr bool FOLD = NT == 3 && RG == 8;        // the idle batch columns 8..15 carry a second term (fold_halves)
  constexpr int PKW = PH / PW;           // K columns per wave
  constexpr int KS = (PKW + 31) / 32;    // k-steps of 32 (the range is zero padded to KS * 32)
  constexpr int KP = KS * 32;
  constexpr int PUC = PH / 32;           // hidden units per CU
  constexpr int MT = (PUC + 3) / 4;      // M tiles: 4 units (16 gate rows) each
  constexpr int HST = KP + 8;            // LDS row stride in bf16: 16-byte multiple, rows 144 B apart at KP = 64 (the 8
                                         // rows of a 16-byte operand read then cover 8 distinct bank groups)
  constexpr int NIMG = FOLD ? 4 : NT;     // folded three terms: + an image that stays zero (the idle half of B2, see fold_halves)
  __shared__ __attribute__((aligned(16))) unsigned short hh[NIMG][PW][RG][HST];    // split terms of the h tile
  __shared__ __attribute__((aligned(16))) float part[2][PW][4 * MT][RG][4];   // K-partials [unit][row][gate], double buffered
  __shared__ int role[2];
  extern __shared__ float occupancy_pad[];                                // forces one workgroup per CU
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i < NIMG * PW * RG * HST; i += PNT) (&hh[0][0][0][0])[i] = 0;   // K padding, unused rows
  int g, slice;
  take_role(a.ctrl, role, g, slice);
  if (slice < 0) return;
  constexpr unsigned spin_limit = FAULT ? DEBUG_SPIN_LIMIT : SPIN_LIMIT;     // (FAULT: persist.h - tests of the abort path)
  const int T = a.T, B = a.B, ndir = a.ndir;
  const int d = ndir == 2 ? (g & 1) : 0;
  const int rowgroup = ndir == 2 ? (g >> 1) : g;
  const int r0 = rowgroup * NR;
  if (r0 >= a.nb) return;                      // this group has no rows (nobody waits for it)
  const int64_t ldy = (int64_t)ndir * PH;
  const int ml = lane & 15, kq = lane >> 4;
  // recurrent weights of this CU -> split bf16 registers
  u32x4 wt[MT][KS][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int grow = 16 * mt + ml;                                  // gate-interleaved row within this CU's 4*PUC
    const bool rok = grow < 4 * PUC;
    const float* wr = a.w + ((int64_t)d * 4 * PH + 4 * PUC * slice + (rok ? grow : 0)) * PH + wave * PKW;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k0 = 32 * ks + 8 * kq;
      float v[8];
#pragma unroll
      for (int j4 = 0; j4 < 2; ++j4) {
        const bool kok = rok && k0 + 4 * j4 < PKW;                  // PKW % 4 == 0: a quad is all in or all out
        const float4 q = *reinterpret_cast<const float4*>(wr + (kok ? k0 + 4 * j4 : 0));
        v[4 * j4] = kok ? q.x : 0.f; v[4 * j4 + 1] = kok ? q.y : 0.f;
        v[4 * j4 + 2] = kok ? q.z : 0.f; v[4 * j4 + 3] = kok ? q.w : 0.f;
      }
      bfn_split8<NT>(v, wt[mt][ks]);
    }
  }
  // pointwise ownership: thread (pu, pj) for tid < PUC*RG -> unit PUC*slice+pu, row r0+pj
  const int pu = tid / RG, pj = tid % RG;
  const bool pw_thread = tid < PUC * RG && pj < NR;
  const int prow = r0 + pj;
  const bool prow_ok = pw_thread && prow < a.nb;
  const int punit = PUC * slice + pu;
  const int plen = prow_ok ? a.lens[prow] : 0;
  // Row of (time, this thread's batch row); see PersistArgs.  PACKED is a template parameter, not a run-time branch: the
  // time-major instantiation must compile from the expression it was tuned with.  These kernels live on the register
  // allocator's goodwill - the forward data of a step is prefetched two steps ahead, and an allocation that cannot give a
  // 16-byte load the four registers its value stays in copies it out of a temporary RIGHT BEHIND the load: a wait for an
  // HBM first touch on the serial chain (bwd 1.80 -> 2.30 us per time step when the run-time form of this map moved it).
  // tools/isa_waits.py lists the vmcnt waits of a kernel's loop; none may follow the prefetch loads.
  const int pbase = (PACKED && prow_ok) ? a.rowbase[prow] : 0;
  const int pext = PACKED ? (prow_ok ? a.rowext[prow] : 1) : a.T;
  // (ROW_AT is a macro, not a lambda: with by-reference captures in the way hipcc allocated the backward kernel's
  // registers differently - see above)
  float c_prev = 0.f;
  float* xw_g = reinterpret_cast<float*>(a.xch) + (int64_t)g * 2 * PH * RG;   // [parity][unit][row]
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(a.xch, 0, 0x7ffffff0, 0x00020000);
  bool aborted = false;
  auto gx_ptr = [&](int sn) {
    const int tt = d == 0 ? sn : T - 1 - sn;
    return reinterpret_cast<const float4*>(a.gates + (ROW_AT(tt) * ndir + d) * 4 * PH + punit * 4);
  };
  float4 gx_n1 = make_float4(0.f, 0.f, 0.f, 0.f), gx_n2 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (prow_ok) {
    gx_n1 = *gx_ptr(0);
    if (T > 1) gx_n2 = *gx_ptr(1);
  }
  float4 st_g = make_float4(0.f, 0.f, 0.f, 0.f);
  float st_c = 0.f, st_y = 0.f;
  float4* st_gp = nullptr;
  int64_t st_so = 0;
  __syncthreads();                             // LDS zero fill
  unsigned abort_seen = 0u;
  for (int s = 0; s < T; ++s) {
    const int t = d == 0 ? s : T - 1 - s;
    LP_MARK(0);
    if (ASR_ABORT_PERIOD_MASK == 0 || (s & ASR_ABORT_PERIOD_MASK) == 0) {      // see lstm_persist_bwd_rs_kernel
      if (pw_thread && flag_load(a.ctrl + 8) != 0u) abort_seen = 1u;
    }
    const float4 gx = gx_n1;
    gx_n1 = gx_n2;
    float4* gp = nullptr;
    if (prow_ok) gp = reinterpret_cast<float4*>(a.gates + (ROW_AT(t) * ndir + d) * 4 * PH + punit * 4);
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // H = 512, 8-row groups, three terms: the wave's h tile as TWO load instructions - k 0-31 and k 32-63 of its range - and
    // the split + products of the first half while the second is still arriving: 1.75 -> 1.68 us per time step against one
    // load per tile, same box, bit-identical results
    constexpr bool HALVES = FOLD && PKW == 64 && NR == 8;
    // the products of k-step ks_ on the staged tile (FOLD form)
#define LP_KSTEP(ks_)                                                                                                  \
    do {                                                                                                               \
      const u32x4 b1 = *reinterpret_cast<const u32x4*>(&hh[ml >> 3][wave][ml & 7][32 * (ks_) + 8 * kq]);                \
      const u32x4 b2 = *reinterpret_cast<const u32x4*>(&hh[2 + (ml >> 3)][wave][ml & 7][32 * (ks_) + 8 * kq]);          \
      _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) acc[mt] = bf3_mfma(wt[mt][ks_][0], b1, acc[mt]);                \
      _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) acc[mt] = bf3_mfma(wt[mt][ks_][1], b1, acc[mt]);                \
      _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) acc[mt] = bf3_mfma(wt[mt][ks_][0], b2, acc[mt]);                \
      _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) acc[mt] = bf3_mfma(wt[mt][ks_][2], b1, acc[mt]);                \
    } while (0)
    if (s > 0) {
      if constexpr (HALVES) {
        // lane l: k = l & 31 of the k-step, rows 4 (l >> 5) .. + 3: ONE quad per lane and k-step, two load instructions in
        // flight; lanes l and l ^ 1 hold adjacent k of the same rows and trade halves (one DPP swap per value), so that
        // every lane splits two (k, k + 1) pairs - rows 0, 1 of its quad on even lanes, rows 2, 3 on odd lanes - and the
        // staging stays 4-byte stores
        const int kk = lane & 31, rh = lane >> 5;
        const unsigned offa = (unsigned)((xw_g - reinterpret_cast<float*>(a.xch)) + ((s - 1) & 1) * (PH * RG) +
                                         (wave * PKW + kk) * RG + 4 * rh) * 4u;
        const unsigned tb = tag_bit_of_step(s - 1);
        u32x4 qa = __builtin_amdgcn_raw_buffer_load_b128(xrs, offa, 0, 16);
        u32x4 qb = __builtin_amdgcn_raw_buffer_load_b128(xrs, offa + 32u * RG * 4u, 0, 16);
        const bool odd = kk & 1;
        const int srow = 4 * rh + (odd ? 2 : 0), scol = kk & ~1;
#define LP_STAGE(q_, ks_)                                                                                              \
        do {                                                                                                           \
          const unsigned t0 = odd ? (q_).x : (q_).z, t1 = odd ? (q_).y : (q_).w;                                       \
          const unsigned r0 = (unsigned)__builtin_amdgcn_mov_dpp((int)t0, 0xB1, 0xF, 0xF, true);   /* quad_perm [1,0,3,2] */ \
          const unsigned r1 = (unsigned)__builtin_amdgcn_mov_dpp((int)t1, 0xB1, 0xF, 0xF, true);                        \
          unsigned tk0[NT], tk1[NT];                                                                                   \
          if (odd) {                                                                                                   \
            bfn_split2<NT>(__uint_as_float(r0), __uint_as_float((q_).z), tk0);                                         \
            bfn_split2<NT>(__uint_as_float(r1), __uint_as_float((q_).w), tk1);                                         \
          } else {                                                                                                     \
            bfn_split2<NT>(__uint_as_float((q_).x), __uint_as_float(r0), tk0);                                         \
            bfn_split2<NT>(__uint_as_float((q_).y), __uint_as_float(r1), tk1);                                         \
          }                                                                                                            \
          _Pragma("unroll") for (int k = 0; k < NT; ++k) {                                                             \
            *reinterpret_cast<unsigned*>(&hh[k][wave][srow][32 * (ks_) + scol]) = tk0[k];                              \
            *reinterpret_cast<unsigned*>(&hh[k][wave][srow + 1][32 * (ks_) + scol]) = tk1[k];                          \
          }                                                                                                            \
        } while (0)
        unsigned spins = 0;
        while (!__all(quad_ok(qa, tb))) {
          if (++spins > spin_limit || ((spins & 63u) == 0u && flag_load(a.ctrl + 8) != 0u)) {
            if (lane == 0) raise_abort(a.ctrl, 1u);
            aborted = true;
            break;
          }
          __builtin_amdgcn_s_sleep(POLL_SLEEP);
          qa = __builtin_amdgcn_raw_buffer_load_b128(xrs, offa, 0, 16);
          qb = __builtin_amdgcn_raw_buffer_load_b128(xrs, offa + 32u * RG * 4u, 0, 16);
        }
        LP_STAGE(qa, 0);
        LP_KSTEP(0);
        while (!aborted && !__all(quad_ok(qb, tb))) {
          if (++spins > spin_limit || ((spins & 63u) == 0u && flag_load(a.ctrl + 8) != 0u)) {
            if (lane == 0) raise_abort(a.ctrl, 1u);
            aborted = true;
            break;
          }
          __builtin_amdgcn_s_sleep(POLL_SLEEP);
          qb = __builtin_amdgcn_raw_buffer_load_b128(xrs, offa + 32u * RG * 4u, 0, 16);
        }
        LP_MARK(7);
        LP_STAGE(qb, 1);
#undef LP_STAGE
      } else if constexpr (NR >= 8) {
        // single-stage hand-off: a lane owns two adjacent k of the wave's range for half of the rows (job = (k pair, row
        // half): 64 jobs at H = 512; H = 640 needs a second job on 16 lanes) and reads them as two 16-byte quads.  The pair is what makes the staging cheap: one packed split (v_cvt_pk_bf16_f32 works on two values
        // anyway) and one 4-byte LDS store per row and term - with one k and all NR rows per lane the same tile took 24
        // two-byte stores per lane (1.85 -> 1.77 us per time step at 8 rows)
        constexpr int RJ = 4;                           // rows per job
        constexpr int NPAIR = PKW / 2, NJOB = NPAIR * (NR / RJ), NJC = (NJOB + 63) / 64;      // (16 rows: four row quarters, two jobs per lane at H = 512)
        static_assert(PKW % 2 == 0, "k pairs");
        bool gl[NJC];
        unsigned boff[NJC];
        int gpair[NJC], ghalf[NJC];
  #pragma unroll
        for (int jc = 0; jc < NJC; ++jc) {
          const int jb = lane + 64 * jc;
          gl[jc] = jb < NJOB;
          ghalf[jc] = gl[jc] ? jb / NPAIR : 0;
          gpair[jc] = gl[jc] ? jb - ghalf[jc] * NPAIR : 0;
          boff[jc] = (unsigned)((xw_g - reinterpret_cast<float*>(a.xch)) + ((s - 1) & 1) * (PH * RG) +
                                (wave * PKW + 2 * gpair[jc]) * RG + RJ * ghalf[jc]) * 4u;
        }
        const unsigned tb = tag_bit_of_step(s - 1);
        unsigned gw[NJC][2][RJ];
        unsigned spins = 0;
        if constexpr (ASR_POLL_SENTINEL_ROWS <= NR) {
          // The poll itself is L2 traffic: every attempt of every wave re-reads its whole tile (32 KB per CU and attempt at 16
          // rows, 1 MB per XCD: ~500 cycles of the L2's bandwidth per round, three rounds per step by the stamps of
          // tools/lstm_trace.py).  So the spin watches ONE quad per lane - a quarter of the tile - and the whole tile is
          // requested once that quad carries this step's tag (its neighbours were written by the same store instruction
          // of the same producer); every word still carries its own tag and is checked below.
          while (true) {
            const u32x4 q = __builtin_amdgcn_raw_buffer_load_b128(xrs, boff[0], 0, 16);
            const bool ok1 = !gl[0] || (((q.x ^ tb) | (q.y ^ tb) | (q.z ^ tb) | (q.w ^ tb)) & 1u) == 0u;
            if (__all(ok1)) break;
            if (++spins > spin_limit || ((spins & 63u) == 0u && flag_load(a.ctrl + 8) != 0u)) break;      // the loop below raises the abort
            __builtin_amdgcn_s_sleep(POLL_SLEEP);
          }
        }
        while (true) {
          bool ok = true;
  #pragma unroll
          for (int jc = 0; jc < NJC; ++jc)
  #pragma unroll
            for (int u = 0; u < 2; ++u) {
              const u32x4 q = __builtin_amdgcn_raw_buffer_load_b128(xrs, boff[jc] + (unsigned)(RG * 4) * u, 0, 16);
              gw[jc][u][0] = q.x; gw[jc][u][1] = q.y; gw[jc][u][2] = q.z; gw[jc][u][3] = q.w;
            }
  #pragma unroll
          for (int jc = 0; jc < NJC; ++jc) {
            unsigned bad = 0u;
  #pragma unroll
            for (int u = 0; u < 2; ++u)
  #pragma unroll
              for (int i = 0; i < RJ; ++i) bad |= gw[jc][u][i] ^ tb;
            ok = ok && (!gl[jc] || (bad & 1u) == 0u);
          }
          if (__all(ok)) break;
          if (++spins > spin_limit || ((spins & 63u) == 0u && flag_load(a.ctrl + 8) != 0u)) {
            if (lane == 0) raise_abort(a.ctrl, 1u);
            aborted = true;
            break;
          }
          __builtin_amdgcn_s_sleep(POLL_SLEEP);
        }
        LP_MARK(7);
  #pragma unroll
        for (int jc = 0; jc < NJC; ++jc)
          if (gl[jc]) {
  #pragma unroll
            for (int i = 0; i < RJ; ++i) {
              unsigned tk[NT];
              bfn_split2<NT>(__uint_as_float(gw[jc][0][i]), __uint_as_float(gw[jc][1][i]), tk);
  #pragma unroll
              for (int k = 0; k < NT; ++k) *reinterpret_cast<unsigned*>(&hh[k][wave][RJ * ghalf[jc] + i][2 * gpair[jc]]) = tk[k];
            }
          }
      } else {
        // 4-row groups: one k per lane, ONE quad - the number of load instructions per lane is what a gather costs
        // (two 8-byte loads per lane for a k pair: 1.51 -> 1.65 us per time step)
        // single-stage hand-off: a lane owns k = lane (+ 64 for H > 512) of the wave's range and reads its 4 rows as
        // 16-byte quads
        constexpr int NKC = (PKW + 63) / 64;
        bool gl[NKC];
        unsigned boff[NKC];
  #pragma unroll
        for (int kc = 0; kc < NKC; ++kc) {
          gl[kc] = lane + 64 * kc < PKW;
          boff[kc] = (unsigned)((xw_g - reinterpret_cast<float*>(a.xch)) + ((s - 1) & 1) * (PH * RG) +
                                (wave * PKW + (gl[kc] ? lane + 64 * kc : 0)) * RG) * 4u;
        }
        const unsigned tb = tag_bit_of_step(s - 1);
        u32x4 gw[NKC][NR / 4];
        unsigned spins = 0;
        while (true) {
  #pragma unroll
          for (int kc = 0; kc < NKC; ++kc)
  #pragma unroll
            for (int j = 0; j < NR / 4; ++j) gw[kc][j] = __builtin_amdgcn_raw_buffer_load_b128(xrs, boff[kc] + 16u * j, 0, 16);
          bool ok = true;
  #pragma unroll
          for (int kc = 0; kc < NKC; ++kc)
  #pragma unroll
            for (int j = 0; j < NR / 4; ++j) ok = ok && (!gl[kc] || quad_ok(gw[kc][j], tb));
          if (__all(ok)) break;
          if (++spins > spin_limit || ((spins & 63u) == 0u && flag_load(a.ctrl + 8) != 0u)) {
            if (lane == 0) raise_abort(a.ctrl, 1u);
            aborted = true;
            break;
          }
          __builtin_amdgcn_s_sleep(POLL_SLEEP);
        }
        LP_MARK(7);
  #pragma unroll
        for (int kc = 0; kc < NKC; ++kc)
          if (gl[kc]) {
  #pragma unroll
            for (int j = 0; j < NR / 4; ++j) {
              const float f[4] = {__uint_as_float(gw[kc][j].x), __uint_as_float(gw[kc][j].y), __uint_as_float(gw[kc][j].z),
                                  __uint_as_float(gw[kc][j].w)};
  #pragma unroll
              for (int i = 0; i < 4; ++i) {
                unsigned tk[NT];
                bfn_split1<NT>(f[i], tk);
  #pragma unroll
                for (int k = 0; k < NT; ++k) hh[k][wave][4 * j + i][lane + 64 * kc] = (unsigned short)tk[k];
              }
            }
          }
      }
      LP_MARK(1);
      if (st_gp) {   // previous step's outputs (stores after the poll: vmcnt retires in order)
        *st_gp = st_g;
        a.c[st_so] = st_c;
        a.y[st_so] = st_y;
        st_gp = nullptr;
      }
      if (prow_ok && s + 2 < T) gx_n2 = *gx_ptr(s + 2);     // in flight for two steps
      // (wave-private LDS tile: program order within the wave is enough)
      if constexpr (HALVES) LP_KSTEP(1);
#pragma unroll
      for (int ks = 0; ks < (HALVES ? 0 : KS); ++ks) {
        if constexpr (FOLD) {
          // columns 8..15 of the batch side carry a second term (fold_halves): four MFMAs per tile and k-step
          const u32x4 b1 = *reinterpret_cast<const u32x4*>(&hh[ml >> 3][wave][ml & 7][32 * ks + 8 * kq]);
          const u32x4 b2 = *reinterpret_cast<const u32x4*>(&hh[2 + (ml >> 3)][wave][ml & 7][32 * ks + 8 * kq]);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[mt] = bf3_mfma(wt[mt][ks][0], b1, acc[mt]);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[mt] = bf3_mfma(wt[mt][ks][1], b1, acc[mt]);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[mt] = bf3_mfma(wt[mt][ks][0], b2, acc[mt]);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[mt] = bf3_mfma(wt[mt][ks][2], b1, acc[mt]);
        } else {
          u32x4 bt[NT];
#pragma unroll
          for (int k = 0; k < NT; ++k) bt[k] = *reinterpret_cast<const u32x4*>(&hh[k][wave][RG == 16 ? ml : (ml & 7)][32 * ks + 8 * kq]);
          // hi hi, hi lo, lo hi
#pragma unroll
          for (int o = 0; o < NT; ++o)
#pragma unroll
            for (int pp = 0; pp <= o; ++pp)
#pragma unroll
              for (int mt = 0; mt < MT; ++mt) acc[mt] = bf3_mfma(wt[mt][ks][pp], bt[o - pp], acc[mt]);
        }
      }
    }
#undef LP_KSTEP
    LP_MARK(2);
    if (s == 0 && prow_ok && T > 2) gx_n2 = *gx_ptr(2);
    if constexpr (FOLD) {
      if (s > 0) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) fold_halves(acc[mt]);
      }
    }
    if (ml < NR) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        *reinterpret_cast<float4*>(&part[s & 1][wave][4 * mt + kq][ml][0]) = make_float4(acc[mt][0], acc[mt][1], acc[mt][2], acc[mt][3]);
    }
    LP_MARK(3);
    __syncthreads();
    LP_MARK(4);
    if (pw_thread) {
      float pre[4] = {gx.x, gx.y, gx.z, gx.w};
#pragma unroll
      for (int w2 = 0; w2 < PW; ++w2) {
        const float4 v = *reinterpret_cast<const float4*>(&part[s & 1][w2][pu][pj][0]);
        pre[0] += v.x; pre[1] += v.y; pre[2] += v.z; pre[3] += v.w;
      }
      const float gi = asr_fast_sigmoid(pre[0]), gf = asr_fast_sigmoid(pre[1]);
      const float gg = asr_fast_tanh(pre[2]), go = asr_fast_sigmoid(pre[3]);
      float cn = gf * c_prev + gi * gg;
      float hn = go * asr_fast_tanh(cn);
      if (t >= plen) { cn = 0.f; hn = 0.f; }
      if (aborted || abort_seen != 0u) hn = __builtin_nanf("");
      c_prev = cn;
      LP_MARK(5);
      if (!(FAULT && g == 0 && slice == 1 && s >= 1))                                                 // (FAULT: a producer that went silent)
        word_store(xw_g + (s & 1) * (PH * RG) + (int64_t)punit * RG + pj, hn, tag_bit_of_step(s));     // hand-off first
      LP_MARK(6);
      if (prow_ok && (!PACKED || t < pext)) {
        st_g = make_float4(gi, gf, gg, go); st_c = cn; st_y = hn;
        st_gp = gp;
        st_so = ROW_AT(t) * ldy + d * PH + punit;
      }
    }
  }
  if (st_gp) {
    // an abort raised elsewhere during the last steps (the flag is sampled every 16th step inside the loop)
    if (flag_load(a.ctrl + 8) != 0u) st_y = __builtin_nanf("");
    *st_gp = st_g;
    a.c[st_so] = st_c;
    a.y[st_so] = st_y;
  }
  // packed rows: the block's padding rows behind the T steps that were run (times T .. rowext - 1; PersistArgs)
  if constexpr (PACKED) if (prow_ok) {
    for (int tt = T; tt < pext; ++tt) {
      const int64_t so = ROW_AT(tt) * ldy + d * PH + punit;
      a.c[so] = 0.f;
      a.y[so] = 0.f;
    }
  }
}

// --------------------------------------------------------------------------------------------------- backward
// The "gathered-dG" backward: dh_rec = dG_{t_next} W_hh for this CU's 16 units, then the pointwise LSTM backward at
// time t (dG_t written in place over the saved gates AND published to the group).  The exchange here is 4x larger
// than in the forward (8 rows x 4H), so it uses bare fp32 words whose mantissa LSB is the validity tag: a slot is
// rewritten every second step and the expected bit flips with every rewrite (the buffer starts zeroed = invalid), so
// a consumer can tell new from stale per word; tearing between words is harmless.  Cost: <= 1 ulp on the exchanged
// copy (the in-place dG used by the weight-gradient GEMMs is untouched).  Float4 traffic both ways.
// One kernel, whose product dh_rec has two forms (`if constexpr (NT == 1)` below; everything else - roles, row map,
// prefetch, hand-off poll and its abort path, pointwise backward, deferred stores, fused dW_hh, db - is shared):
//   NT = 1       exact fp32 on v_mfma_f32_4x4x1f32.  MFMA blocks: 16 = 4 unit-groups x 4 k-subs; A[blk][i] =
//                W_hhT[unit 4ug+i][k], B[blk][j] = dG[row j][k], k = 256*wave + 64*ks + q.  The 4 k-sub partials are
//                summed with DPP, the 8 waves' partials by the pointwise thread.
//   NT = 2 / 3   v_mfma_f32_16x16x32_bf16, operands split in NT bf16 terms as in lstm_persist_fwd_bf3_kernel (three /
//                six products, fp32 accumulation): A = this CU's 16 units of W_hh^T in registers, B = the gathered dG
//                tile, which the gathering lanes write to LDS twice - as fp32 for the fused dW_hh product (unchanged,
//                exact fp32, off the serial chain) and split in bf16 for this one.

template <int PH, int NR, int NT, bool PACKED = false>
__global__ __launch_bounds__(PNT) void lstm_persist_bwd_kernel(PersistArgs a) {
  static_assert(NR == 4 || NR == PRG, "rows per group (see the forward kernel)");
  static_assert(NT >= 1 && NT <= 3, "1: fp32 operands, 2 / 3: split-bf16 terms");
  constexpr int PUC = PH / 32;       // hidden units per CU
  constexpr int PKB = 4 * PH / PW;   // gate columns per wave
  constexpr int PQ = PKB / 4;        // k's per (wave, k-sub)
  constexpr int PQS = PQ + 4;        // padded LDS stride of a k-sub chunk
  constexpr int KSB = PKB / 32;      // split form: k-steps of the dh product
  constexpr int BST = PKB + 8;       // split form: bf16 row stride (16-byte multiple, 8 rows of a read on distinct bank groups)
  // this wave's K range of dG as [row][k-sub][64 + 4]: the 16 distinct (k-sub, row) addresses of one ds_read_b128
  // differ by 68*ks + 272*row floats = 16 distinct 16-B bank slots (unpadded they are all 256-B multiples: 16-way).
  // The fp32 copy of the tile: operand of dW_hh in both forms, of the dh product with NT = 1.
  __shared__ __attribute__((aligned(16))) float hs[PW][PRG][4 * PQS];
  // partial dh_rec, double buffered: NT = 1 [lane][register] of the 4x4x1 blocks (36 KB), split form [row][unit]
  __shared__ __attribute__((aligned(NT == 1 ? 4 : 16))) float part[2][PW][NT == 1 ? 64 : PRG][NT == 1 ? 9 : 16];
  // the dG tile split in NT bf16 terms, B operand of the split product.  With NT = 1 an empty type that nothing names: it
  // takes no LDS (the lds_bytes column of tests/golden/isa_table.json)
  struct NoTile {};
  __shared__ __attribute__((aligned(16))) std::conditional_t<NT == 1, NoTile, unsigned short[NT][PW][PRG][BST]> bsp;
  __shared__ float ysl[2][PRG][16];                                       // this CU's slice of h at the current time
  __shared__ int role[2];
  constexpr int NKQ = (PKB + 63) / 64;                                    // 64-column chunks of the wave's K range
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < 2 * PRG * 16) (&ysl[0][0][0])[tid] = 0.f;
  if constexpr (NT > 1) {
    static_assert(PKB % 32 == 0 && PUC <= 16, "one 16-unit M tile, whole k-steps");
    for (int i = tid; i < NT * PW * PRG * BST; i += PNT) (&bsp[0][0][0][0])[i] = 0;   // rows >= NR stay 0
  }
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int g, slice;
  take_role(a.ctrl, role, g, slice);
  if (slice < 0) return;
  const int T = a.T, B = a.B, ndir = a.ndir;
  const int d = ndir == 2 ? (g & 1) : 0;
  const int rowgroup = ndir == 2 ? (g >> 1) : g;
  const int r0 = rowgroup * NR;
  if (r0 >= a.nb) return;
  const int64_t ldy = (int64_t)ndir * PH, ldg = (int64_t)ndir * 4 * PH;
  // lane maps of the dh product.  NT = 1: lane (ug = lane>>4, ks = (lane>>2)&3, li = lane&3) holds unit 16*slice+4ug+li,
  // k = 256*wave + 64*ks + q, q = 0..63.  Split form: lane l holds unit ml = l & 15 of this CU, gate columns
  // wave*PKB + 32 kt + 8 kg + j, kg = l >> 4 (A operand of the 16x16x32 product).
  const int ug = lane >> 4, ks = (lane >> 2) & 3, li = lane & 3;
  const int ml = lane & 15, kg = lane >> 4;
  // W_hhT slice -> registers for the whole sequence: fp32 words, or split bf16 per k-step
  std::conditional_t<NT == 1, float[PQ], u32x4[KSB][NT]> wreg;
  if constexpr (NT == 1) {
    const int wu = 4 * ug + li < PUC ? 4 * ug + li : 0;     // unit groups beyond PUC idle
    const float* wr = a.w + ((int64_t)d * PH + PUC * slice + wu) * (4 * PH) + wave * PKB + PQ * ks;
#pragma unroll
    for (int q4 = 0; q4 < PQ / 4; ++q4) {
      const float4 v = *reinterpret_cast<const float4*>(wr + 4 * q4);
      wreg[4 * q4] = v.x; wreg[4 * q4 + 1] = v.y; wreg[4 * q4 + 2] = v.z; wreg[4 * q4 + 3] = v.w;
    }
  } else {
    const bool uok = ml < PUC;
    const float* wr = a.w + ((int64_t)d * PH + PUC * slice + (uok ? ml : 0)) * (4 * PH) + wave * PKB + 8 * kg;
#pragma unroll
    for (int kt = 0; kt < KSB; ++kt) {
      const float4 q0 = *reinterpret_cast<const float4*>(wr + 32 * kt), q1 = *reinterpret_cast<const float4*>(wr + 32 * kt + 4);
      const float v[8] = {uok ? q0.x : 0.f, uok ? q0.y : 0.f, uok ? q0.z : 0.f, uok ? q0.w : 0.f,
                          uok ? q1.x : 0.f, uok ? q1.y : 0.f, uok ? q1.z : 0.f, uok ? q1.w : 0.f};
      bfn_split8<NT>(v, wreg[kt]);
    }
  }
  // Waves 6-7 mirror the pointwise threads' (unit, row) mapping: they issue the SAME forward-data loads two steps
  // further ahead and discard them, which pulls those HBM rows into this XCD's L2 before the pointwise threads ask
  // (their own loads, one step ahead, were HBM first touches: ~0.3 us of every step with a cached row, see DESIGN).
  const int mt = tid & 127;
  const int pu = mt >> 3, pj = mt & 7;
  const bool pw_lane = tid < PUC * PRG;                 // all 8 row lanes of a unit (bias-gradient reduction)
  const bool pw_thread = pw_lane && pj < NR;
  const int prow = r0 + pj;
  const bool prow_ok = pw_thread && prow < a.nb;
  const bool touch_ok = ASR_LSTM_TOUCH && tid >= 384 && mt < PUC * PRG && pj < NR && prow < a.nb;
  const int punit = PUC * slice + pu;
  const int plen = prow_ok ? a.lens[prow] : 0;
  // row of (time, this thread's batch row): see PersistArgs and the note in lstm_persist_bwd_rs_kernel
  const int pbase = (PACKED && prow_ok) ? a.rowbase[prow] : 0;
  const int pext = PACKED ? (prow_ok ? a.rowext[prow] : 1) : a.T;
  float dcarry = 0.f;
  float4 dbacc = make_float4(0.f, 0.f, 0.f, 0.f);   // bias gradient of this thread's (unit, row): sum of dG over time
  float* xch_g = reinterpret_cast<float*>(a.xch) + (int64_t)g * PRG * 4 * PH;   // + parity * 8*PRG*4H
  const int64_t par_stride = (int64_t)8 * PRG * 4 * PH;
  typedef unsigned u4v __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(a.xch, 0, 0x7ffffff0, 0x00020000);   // raw dwords
  bool aborted = false;
  // pointwise operands are fetched one step ahead (see the forward kernel)
  float n_dy = 0.f, n_ct = 0.f, n_cp = 0.f, n_y = 0.f;
  float4 n_av = make_float4(0.f, 0.f, 0.f, 0.f);
  const bool fuse_dw = a.dw != nullptr && a.yfwd != nullptr;
  // dW_hh accumulators: [64-column chunk][unit group] 4x4 blocks, kept in registers for the whole sequence
  f32x4 dwacc[NKQ][4];
#pragma unroll
  for (int kq = 0; kq < NKQ; ++kq)
#pragma unroll
    for (int u4 = 0; u4 < 4; ++u4) dwacc[kq][u4] = (f32x4){0.f, 0.f, 0.f, 0.f};
  auto fetch_step = [&](int sn) {
    const int tt = d == 0 ? T - 1 - sn : sn;
    const int ttp = d == 0 ? tt - 1 : tt + 1;
    const bool hp = d == 0 ? (tt > 0) : (tt < T - 1);
    const int64_t so = ROW_AT(tt) * ldy + d * PH + punit;
    n_dy = a.dy[so];
    n_av = *reinterpret_cast<const float4*>(a.gates + ROW_AT(tt) * ldg + (int64_t)d * 4 * PH + punit * 4);
    n_ct = a.c[so];
    n_cp = hp ? a.c[ROW_AT(ttp) * ldy + d * PH + punit] : 0.f;
    if (fuse_dw) n_y = a.yfwd[so];
  };
  if (prow_ok) fetch_step(0);
  for (int s = 0; s < T; ++s) {
    const int t = d == 0 ? T - 1 - s : s;
    LP_MARK(0);
    const unsigned abort_seen = pw_thread ? flag_load(a.ctrl + 8) : 0u;     // see the forward kernel
    const float dyv = n_dy, ct = n_ct, cp = n_cp;
    const float4 av = n_av;
    float4* gp = nullptr;
    if (prow_ok) gp = reinterpret_cast<float4*>(a.gates + ROW_AT(t) * ldg + (int64_t)d * 4 * PH + punit * 4);
    if (fuse_dw && pw_thread) ysl[s & 1][pj][pu] = prow_ok ? n_y : 0.f;     // h_t of this CU's units (read after the barrier)
    // NT = 1: two alternating accumulators; split form: three independent ones (one per group of split products)
    f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc2 = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (s > 0) {
      const unsigned want = (((unsigned)(s - 1) >> 1) & 1u) ^ 1u;      // tag bit of the data written at step s-1
      const bool gl = 4 * lane < PKB;                   // lanes beyond the wave's K range re-read column 0
      const float* src = xch_g + ((s - 1) & 1) * par_stride + wave * PKB + (gl ? 4 * lane : 0);
      float4 gr[NR];
      unsigned spins = 0;
      auto load_row = [&](int rr) {
        // L1-bypassing 16-byte read in ONE instruction: buffer load with the sc1 cache policy (the same policy the
        // agent-scope atomic loads get, which exist only up to 8 bytes)
        const u4v v = __builtin_amdgcn_raw_buffer_load_b128(
            xrs, (unsigned)((src - reinterpret_cast<const float*>(a.xch)) + rr * 4 * PH) * 4u, 0, 16);
        gr[rr].x = __uint_as_float(v.x); gr[rr].y = __uint_as_float(v.y);
        gr[rr].z = __uint_as_float(v.z); gr[rr].w = __uint_as_float(v.w);
      };
      auto row_bits = [&](int rr) -> unsigned {
        const unsigned m = (__float_as_uint(gr[rr].x) & 1u) | ((__float_as_uint(gr[rr].y) & 1u) << 1) |
                           ((__float_as_uint(gr[rr].z) & 1u) << 2) | ((__float_as_uint(gr[rr].w) & 1u) << 3);
        return want ? m : (~m & 0xFu);
      };
      bool first = wave < ASR_LSTM_BWD_FULL_WAVES;
      while (true) {
        if (first) {
          // the pointwise waves poll last: first attempt requests the whole tile at once (one L2 round trip); as a
          // separate code path -- folded into the sentinel condition the compiler still waited for the sentinel
          first = false;
#pragma unroll
          for (int rr = 0; rr < NR; ++rr) load_row(rr);
          unsigned bits = 0xFu;
#pragma unroll
          for (int rr = 0; rr < NR; ++rr) bits &= row_bits(rr);
          if (__all(!gl || bits == 0xFu)) break;
        } else {
          // cheap sentinel poll: the last row of this wave's K range (1 KB, touches all 4 producer CUs); a failed
          // poll of the whole 64 KB per CU would saturate the XCD's L2 and delay the producers themselves
          load_row(NR - 1);
          bool ok = !gl || row_bits(NR - 1) == 0xFu;
          if (__all(ok)) {
#pragma unroll
            for (int rr = 0; rr < NR - 1; ++rr) load_row(rr);
            unsigned bits = row_bits(NR - 1);
#pragma unroll
            for (int rr = 0; rr < NR - 1; ++rr) bits &= row_bits(rr);
            if (__all(!gl || bits == 0xFu)) break;
          }
        }
        if (++spins > SPIN_LIMIT || ((spins & 63u) == 0u && flag_load(a.ctrl + 8) != 0u)) {
          if (lane == 0) raise_abort(a.ctrl, 3u);
          aborted = true;
          break;
        }
        __builtin_amdgcn_s_sleep(POLL_SLEEP);
      }
      LP_MARK(1);
#pragma unroll
      for (int rr = 0; rr < NR; ++rr)
        if (gl) {
          *reinterpret_cast<float4*>(&hs[wave][rr][PQS * ((4 * lane) / PQ) + (4 * lane) % PQ]) = gr[rr];
          if constexpr (NT > 1) {
            unsigned p0[NT], p1[NT];
            bfn_split2<NT>(gr[rr].x, gr[rr].y, p0);
            bfn_split2<NT>(gr[rr].z, gr[rr].w, p1);
#pragma unroll
            for (int k = 0; k < NT; ++k) *reinterpret_cast<uint2*>(&bsp[k][wave][rr][4 * lane]) = make_uint2(p0[k], p1[k]);
          }
        }
      if (prow_ok && s + 1 < T) fetch_step(s + 1);
      else if (touch_ok && s + ASR_LSTM_TOUCH_DIST < T) fetch_step(s + ASR_LSTM_TOUCH_DIST);   // L2 warm-up (results unused)
      if constexpr (NT == 1) {
        const float* h0 = &hs[wave][li][PQS * ks];
        const float* h1 = &hs[wave][4 + li][PQS * ks];
#pragma unroll
        for (int q4 = 0; q4 < PQ / 4; ++q4) {
          const float4 b0 = *reinterpret_cast<const float4*>(h0 + 4 * q4);
          if (NR > 4) {                      // alternating accumulators, see the forward kernel
            const float4 b1 = *reinterpret_cast<const float4*>(h1 + 4 * q4);
            acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * q4], b0.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * q4], b1.x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * q4 + 1], b0.y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * q4 + 1], b1.y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * q4 + 2], b0.z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * q4 + 2], b1.z, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * q4 + 3], b0.w, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * q4 + 3], b1.w, acc1, 0, 0, 0);
          } else {
            acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * q4], b0.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * q4 + 1], b0.y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * q4 + 2], b0.z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(wreg[4 * q4 + 3], b0.w, acc1, 0, 0, 0);
          }
        }
        if (NR <= 4) {
#pragma unroll
          for (int i = 0; i < 4; ++i) acc0[i] += acc1[i];
        }
      } else {
        // dh partial [16 units x rows] of this wave's K range
#pragma unroll
        for (int kt = 0; kt < KSB; ++kt) {
          u32x4 bt[NT];
#pragma unroll
          for (int k = 0; k < NT; ++k) bt[k] = *reinterpret_cast<const u32x4*>(&bsp[k][wave][ml & 7][32 * kt + 8 * kg]);
          acc0 = bf3_mfma(wreg[kt][0], bt[0], acc0);
          acc1 = bf3_mfma(wreg[kt][0], bt[1], acc1);
          acc2 = bf3_mfma(wreg[kt][1], bt[0], acc2);
          if constexpr (NT == 3) {
            acc0 = bf3_mfma(wreg[kt][0], bt[2], acc0);
            acc1 = bf3_mfma(wreg[kt][2], bt[0], acc1);
            acc2 = bf3_mfma(wreg[kt][1], bt[1], acc2);
          }
        }
      }
    }
    if (s == 0 && prow_ok && T > 1) fetch_step(1);
    LP_MARK(2);
    if constexpr (NT == 1) {
      // the 4 k-sub partials of a (unit, row) sit 4 lanes apart inside a row of 16: two DPP row rotations leave their
      // sum in every one of those lanes, so the pointwise thread reads 8 values (one per wave) instead of 32.  (Done on
      // scalar copies: applied to the elements of the MFMA accumulator vector in place, hipcc 7.2 paired the rotations
      // with the wrong elements.)
      float red[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) { red[i] = acc0[i]; red[4 + i] = NR > 4 ? acc1[i] : 0.f; }
#pragma unroll
      for (int i = 0; i < (NR > 4 ? 8 : 4); ++i) {
        red[i] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, red[i]), 0x124, 0xf, 0xf, true));
        red[i] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, red[i]), 0x128, 0xf, 0xf, true));
      }
      float* pp = &part[s & 1][wave][lane][0];
#pragma unroll
      for (int i = 0; i < (NR > 4 ? 8 : 4); ++i) pp[i] = red[i];
    } else {
      // D of the 16x16x32 product puts the 4 units 4 (l >> 4) .. + 3 of batch row l & 15 in one lane: the 4 k-sub
      // partials of the 4x4x1 mapping and their DPP reduction are gone
      if (ml < NR)
        *reinterpret_cast<float4*>(&part[s & 1][wave][ml][4 * kg]) =
            make_float4(acc0[0] + acc1[0] + acc2[0], acc0[1] + acc1[1] + acc2[1], acc0[2] + acc1[2] + acc2[2],
                        acc0[3] + acc1[3] + acc2[3]);
    }
    LP_MARK(3);
    __syncthreads();
    LP_MARK(4);
    if (pw_thread) {
      float dh = dyv;
      if constexpr (NT == 1) {
        // dh_rec[unit pu][row pj]: lanes 16*(pu>>2) + 4*ks + (pj&3), register 4*(pj>>2) + (pu&3), all waves
        const int pl = 16 * (pu >> 2) + (pj & 3), pr = 4 * (pj >> 2) + (pu & 3);
#pragma unroll
        for (int w2 = 0; w2 < PW; ++w2) dh += part[s & 1][w2][pl][pr];      // k-subs already summed (DPP, above)
      } else {
#pragma unroll
        for (int w2 = 0; w2 < PW; ++w2) dh += part[s & 1][w2][pj][pu];
      }
      LP_MARK(9);
      const float tc = asr_fast_tanh(ct);
      const float dc = dcarry + dh * av.w * (1.f - tc * tc);
      float4 da;
      da.x = dc * av.z * av.x * (1.f - av.x);
      da.y = dc * cp * av.y * (1.f - av.y);
      da.z = dc * av.x * (1.f - av.z * av.z);
      da.w = dh * tc * av.w * (1.f - av.w);
      float dcn = dc * av.y;
      if (t >= plen) { da = make_float4(0.f, 0.f, 0.f, 0.f); dcn = 0.f; }
      if (aborted || abort_seen != 0u) da.x = __builtin_nanf("");
      dcarry = dcn;
      const unsigned bit = (((unsigned)s >> 1) & 1u) ^ 1u;
      float4 tg;
      tg.x = tag_word(da.x, bit); tg.y = tag_word(da.y, bit); tg.z = tag_word(da.z, bit); tg.w = tag_word(da.w, bit);
      LP_MARK(10);
      float* dst = xch_g + (s & 1) * par_stride + (int64_t)pj * 4 * PH + punit * 4;
      // two 8-byte workgroup-scope (plain, L2-resident) stores; every word carries its own tag
      __hip_atomic_store((gu64*)dst, ((u64)__float_as_uint(tg.y) << 32) | __float_as_uint(tg.x), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_store((gu64*)dst + 1, ((u64)__float_as_uint(tg.w) << 32) | __float_as_uint(tg.z), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_WORKGROUP);
      LP_MARK(11);
      if (prow_ok) {     // after the hand-off: the bulk store and the bias-gradient sum are off the serial chain
        if (!PACKED || t < pext) *gp = da;
        dbacc.x += da.x; dbacc.y += da.y; dbacc.z += da.z; dbacc.w += da.w;
      }
    }
    LP_MARK(5);
    // Fused recurrent weight gradient: dW_hh[k][u] += sum_rows dG_{t_next}[row][k] * h_t[row][u].  The gathered dG
    // tile is still in this wave's LDS region and h_t is the partner of dG_{t_next} in both directions.  Placed
    // after the publish so that it fills the wait for the next hand-off.  Blocks = 16 groups of 4 gate columns,
    // A = dG (4 columns), B = h (4 units), K = one batch row per instruction.
    if (fuse_dw && s > 0) {
      const int kb4 = lane;                      // column within the 64-column chunk (= 4*block + i)
      const int jj = lane & 3;
#pragma unroll
      for (int rr = 0; rr < NR; ++rr) {
        float bv[4];
#pragma unroll
        for (int u4 = 0; u4 < 4; ++u4) bv[u4] = ysl[s & 1][rr][4 * u4 + jj];
#pragma unroll
        for (int kq = 0; kq < NKQ; ++kq) {
          const int cidx = 64 * kq + kb4;
          const float av2 = cidx < PKB ? hs[wave][rr][PQS * (cidx / PQ) + cidx % PQ] : 0.f;
#pragma unroll
          for (int u4 = 0; u4 < 4; ++u4)
            dwacc[kq][u4] = __builtin_amdgcn_mfma_f32_4x4x1f32(av2, bv[u4], dwacc[kq][u4], 0, 0, 0);
        }
      }
    }
  }
  // packed rows: dG of the block's padding rows behind the T steps that were run (PersistArgs)
  if constexpr (PACKED) if (prow_ok) {
    for (int tt = T; tt < pext; ++tt)
      *reinterpret_cast<float4*>(a.gates + ROW_AT(tt) * ldg + (int64_t)d * 4 * PH + punit * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (a.db != nullptr && pw_lane) {
    // rows of a unit sit in 8 consecutive lanes (pj = tid & 7); the 4 row groups (XCDs) of a direction add up
    float v[4] = {dbacc.x, dbacc.y, dbacc.z, dbacc.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] += __shfl_xor(v[k], 1, 64);
      v[k] += __shfl_xor(v[k], 2, 64);
      v[k] += __shfl_xor(v[k], 4, 64);
    }
    if (pj == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) atomicAdd(a.db + (int64_t)d * 4 * PH + punit * 4 + k, v[k]);
    }
  }
  if (fuse_dw) {
    // D[i][j] of block kb: gate column 64*kq + 4*kb + i of this wave's range, unit 4*u4 + j of this CU; the 4 row
    // groups (XCDs) of a direction add into the same dW_hh
    const int kb = lane >> 2, jj = lane & 3;
#pragma unroll
    for (int kq = 0; kq < NKQ; ++kq)
#pragma unroll
      for (int u4 = 0; u4 < 4; ++u4)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int cidx = 64 * kq + 4 * kb + i, un = 4 * u4 + jj;
          if (cidx < PKB && un < PUC)
            atomicAdd(a.dw + ((int64_t)d * 4 * PH + wave * PKB + cidx) * PH + PUC * slice + un, dwacc[kq][u4][i]);
        }
  }
}

// ------------------------------------------------------------- backward, exchanged dh partials ("reduce-scatter")
// The kernels above hand the step's dG (8 rows x 4H) to all 32 CUs of the group: every CU gathers 64 KB per time step
// (2 MB through the XCD's L2), which is what a backward step waits for (tools/lstm_trace.py: 1 600 cycles from the top
// of a step to its tile, another 2 500 to stage, convert and multiply it).  dG is the wide side of the product
// dh_rec[row][unit] = sum_col dG[row][col] W_hh[col][unit]; this kernel exchanges the narrow one:
//   * CU j keeps the dG columns of its OWN units (it produces them in the pointwise phase: 8 rows x 64 columns that
//     never leave the CU) and the matching 64 rows of W_hh for ALL units (split bf16, registers);
//   * per step it forms the partial dh of all H units from those columns (K = 64: two k-steps of
//     v_mfma_f32_16x16x32_bf16 per 16-unit tile, 3 split products) and publishes it as LSB-tagged fp32 quads, laid out
//     [dest CU][source CU][row][unit]: 16 KB written, and each CU then gathers the 16 KB addressed to it
//     (32 sources x 8 rows x 16 units) - a quarter of the old gather, no operand conversion on the consumer side - and
//     sums the 32 sources with DPP adds inside half waves;
//   * dW_hh[col][unit] += sum_rows dG_t[row][col] h_{t_prev}[row][unit] for the CU's 64 columns x all H units: dG is
//     local, h_{t_prev} is forward data (8 rows x H, prefetched a step ahead); the product runs on
//     v_mfma_f32_16x16x16_bf16 (K = 8 batch rows, zero padded to 16), split in three like the others: 768 MFMA cycles
//     per SIMD and step instead of 2 048 on the fp32 pipe, and it sits between the publish and the next gather.
// H in {128, 256, 512} (units per CU a multiple of 4); other sizes keep lstm_persist_bwd_kernel.
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
__device__ __forceinline__ f32x4 bf3_mfma16(const uint2& a, const uint2& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a), __builtin_bit_cast(s16x4, b), c, 0, 0, 0);
}

template <int PH>
struct RsDims {
  // Units per CU: PUR real ones; the exchange, the MFMA tiles and the (row, unit quad) gather work on PUC = PUR rounded up
  // to a multiple of 4.  H = 320 (config.yaml's own width): 10 real units in 12 slots per CU - a padded unit has zero
  // weights, is never computed by the pointwise threads and never reaches memory; the padded hidden size PHP = 384 is what
  // the tile counts below follow.  (Unfused three-term kernel only: the fused dW_hh path indexes h by storage unit.)
  static constexpr int PUR = PH / 32;
  static constexpr int PUC = (PUR + 3) / 4 * 4;
  static constexpr int PHP = 32 * PUC;
  static constexpr int NCR = 4 * PUR;            // real local gate columns
  static constexpr int NC = 4 * PUC;             // local gate columns
  static constexpr int KS = (NC + 31) / 32;      // k-steps of the dh-partial product
  static constexpr int KP = KS * 32;
  static constexpr int MTW = (PHP / 16) / PW;    // 16-unit tiles per wave (dh partial M tiles = dW unit tiles)
  static constexpr int CT = (NC + 15) / 16;      // 16-column tiles of dW
  static constexpr int UPW = PHP / PW;           // units per wave
  static constexpr int CPW = PUC / 4;            // (row, unit-quad) combos gathered per wave
  static constexpr int QPU = PUC / 4;            // unit quads per (source, row)
  static constexpr int GST = KP + 8;             // bf16 row stride of the row-major local dG
  static constexpr size_t group_floats = (size_t)2 * 32 * 32 * PRG * PUC;     // exchange per group (both parities)
  static_assert(PH % 32 == 0 && PHP % 128 == 0 && PUC <= 16, "H in {128, 256, 320, 512}");
};

template <int PH, int NR, int NT, bool PACKED = false>
__global__ __launch_bounds__(PNT) void lstm_persist_bwd_rs_kernel(PersistArgs a) {
  using RD = RsDims<PH>;
  constexpr int PUC = RD::PUC, PUR = RD::PUR, NC = RD::NC, NCR = RD::NCR, KS = RD::KS, MTW = RD::MTW, CT = RD::CT, UPW = RD::UPW, CPW = RD::CPW;
  constexpr int QPU = RD::QPU, GST = RD::GST;
  constexpr int NE = 2;                           // quads per lane in the gather: two sources of one (row, unit quad)
  // local dG of the last four steps, row-major [slot s & 3][row][col] (split bf16).  One image serves both products:
  //   dh partial (this step):  B operand = 8 consecutive columns of a row            -> ds_read_b128
  //   dW_hh (every third step): A operand = 8 rows (k = slot * 8 + row) of a column  -> two ds_read_b64_tr_b16 (the
  //     hardware transpose read, tools/micro/tr_read_check.hip)
  // The first version kept a second, column-major copy for dW_hh that the pointwise threads filled with 24 two-byte LDS
  // stores per step: 0.13 us of the serial chain.  h_{t_prev} stays [unit][slot][row].
  // Three terms (NT = 3, six products per product): dW_hh is NOT fused.  With three terms of W in registers (96 VGPRs)
  // the 64 accumulator registers of dW_hh do not fit, and a first version that kept the third term of W in LDS and the h
  // tile as fp32 measured the fused product at 1.08 us per time step (2 x the MFMAs of the two-term form, all of it on
  // the serial chain: every CU is producer and consumer) - 1.5 ms per cfg-2 step, against 1.2 ms for the same sums as two
  // batched 256 x 128 GEMMs after the kernel (ops._LstmLayer).  FUSE is therefore a property of the two-term kernel.
  constexpr bool FUSE = NT == 2;
  static_assert(!FUSE || PUR == PUC, "padded units per CU exist in the unfused kernel only");
  constexpr int NIMG = NT == 3 ? 4 : NT;  // three terms: + an image that stays zero (the idle half of B2, see fold_halves)
  __shared__ __attribute__((aligned(16))) unsigned short dgs[NIMG][FUSE ? 4 : 2][PRG][GST];
  __shared__ __attribute__((aligned(16))) unsigned short ht2[FUSE ? 2 : 1][FUSE ? PH : 1][4][PRG];
  __shared__ __attribute__((aligned(16))) float dbs[PRG][4 * PUC];                            // bias-gradient sums per row (epilogue)
  __shared__ __attribute__((aligned(16))) float dhs[PRG][16];                                 // reduced dh_rec [row][unit] (fused kernel)
  __shared__ int role[2];
  extern __shared__ float occupancy_pad[];                                // forces one workgroup per CU
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i < NIMG * (FUSE ? 4 : 2) * PRG * GST; i += PNT) (&dgs[0][0][0][0])[i] = 0;
  if constexpr (FUSE) {
    for (int i = tid; i < 2 * PH * 4 * PRG; i += PNT) (&ht2[0][0][0][0])[i] = 0;
  }
  for (int i = tid; i < PRG * 4 * PUC; i += PNT) (&dbs[0][0])[i] = 0.f;
  int g, slice;
  take_role(a.ctrl, role, g, slice);
  if (slice < 0) return;
  const int T = a.T, B = a.B, ndir = a.ndir;
  const int d = ndir == 2 ? (g & 1) : 0;
  const int rowgroup = ndir == 2 ? (g >> 1) : g;
  const int r0 = rowgroup * NR;
  if (r0 >= a.nb) return;
  const int64_t ldy = (int64_t)ndir * PH, ldg = (int64_t)ndir * 4 * PH;
  const int ml = lane & 15, kq = lane >> 4;
  // W_hh rows of this CU's columns, all units -> split bf16: A operand of the dh-partial product.  a.w is W_hh^T
  // [unit][4H]: lane l holds unit 16 (MTW wave + mt) + (l & 15), columns NC slice + 32 ks + 8 (l >> 4) + j
  u32x4 wt[MTW][KS][NT];
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt) {
    const int cu = 16 * (MTW * wave + mt) + ml;                     // unit slot (padded index); its owner CU and slot there
    const int csl = cu / PUC, cuu = cu - csl * PUC;
    const bool ureal = cuu < PUR;
    const int wunit = PUR * csl + (ureal ? cuu : 0);                // storage unit
    const float* wr = a.w + ((int64_t)d * PH + wunit) * (4 * PH) + NCR * slice;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k0 = 32 * ks + 8 * kq;
      float v[8];
      if (a.w_il != nullptr) {      // forward layout [4H columns][H units]: the same elements, one at a time (once per launch)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool kok = ureal && k0 + j < NCR;
          const float q = a.w_il[((int64_t)d * 4 * PH + NCR * slice + (kok ? k0 + j : 0)) * PH + wunit];
          v[j] = kok ? q : 0.f;
        }
      } else {
#pragma unroll
        for (int j4 = 0; j4 < 2; ++j4) {
          const bool kok = ureal && k0 + 4 * j4 < NCR;
          const float4 q = *reinterpret_cast<const float4*>(wr + (kok ? k0 + 4 * j4 : 0));
          v[4 * j4] = kok ? q.x : 0.f; v[4 * j4 + 1] = kok ? q.y : 0.f;
          v[4 * j4 + 2] = kok ? q.z : 0.f; v[4 * j4 + 3] = kok ? q.w : 0.f;
        }
      }
      bfn_split8<NT>(v, wt[mt][ks]);
    }
  }
  // Pointwise ownership.  Unfused kernel (ROWPW): it follows the gather - the 16 lanes of DPP row rr of wave w sum the 32
  // partials of (row w, unit quad rr), every lane of the row ends up with the four totals, and lanes 0..3 of the row go on
  // with the pointwise backward of (row w, unit 4 rr + lane) on the spot: no LDS round trip of the reduced dh, no barrier
  // between gather and pointwise phase, two alternating dG slots instead (1.88 -> 1.83 us per time step).  The fused
  // two-term kernel keeps the first mapping, thread (pu, pj) of waves 0 and 1 behind barrier A: its dW_hh block needs that
  // barrier anyway, and with the pointwise code in all eight waves it measured 2.17 instead of 2.02 us.
  constexpr bool ROWPW = !FUSE;
  static_assert(QPU == CPW, "a wave gathers exactly one row");
  const int rr = lane >> 4, sp = lane & 15;
  const int pu = ROWPW ? 4 * (rr < CPW ? rr : 0) + (sp & 3) : tid >> 3, pj = ROWPW ? wave : tid & 7;
  const bool pw_lane = ROWPW ? (sp < 4 && rr < CPW && pu < PUR) : tid < PUR * PRG;
  const bool pw_thread = pw_lane && pj < NR;
  const int prow = r0 + pj;
  const bool prow_ok = pw_thread && prow < a.nb;
  const int punit = PUR * slice + pu;
  const int plen = prow_ok ? a.lens[prow] : 0;
  // Row of (time, this thread's batch row); see PersistArgs.  PACKED is a template parameter, not a run-time branch: the
  // time-major instantiation must compile from the expression it was tuned with.  These kernels live on the register
  // allocator's goodwill - the forward data of a step is prefetched two steps ahead, and an allocation that cannot give a
  // 16-byte load the four registers its value stays in copies it out of a temporary RIGHT BEHIND the load: a wait for an
  // HBM first touch on the serial chain (bwd 1.80 -> 2.30 us per time step when the run-time form of this map moved it).
  // tools/isa_waits.py lists the vmcnt waits of a kernel's loop; none may follow the prefetch loads.
  const int pbase = (PACKED && prow_ok) ? a.rowbase[prow] : 0;
  const int pext = PACKED ? (prow_ok ? a.rowext[prow] : 1) : a.T;
  // (ROW_AT is a macro, not a lambda: with by-reference captures in the way hipcc allocated the backward kernel's
  // registers differently - see above)
  float dcarry = 0.f;
  float4 dbacc = make_float4(0.f, 0.f, 0.f, 0.f);
  float* xg = reinterpret_cast<float*>(a.xch) + (int64_t)g * RD::group_floats;
  constexpr int PARSZ = 32 * 32 * PRG * PUC;      // floats per parity
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(a.xch, 0, 0x7ffffff0, 0x00020000);
  bool aborted = false;
  const bool fuse_dw = FUSE && a.dw != nullptr && a.yfwd != nullptr;
  // gather role: the 16 lanes of DPP row rr = lane >> 4 sum the 32 sources of combo CPW wave + rr = (row, unit quad), two
  // sources (2 sp, 2 sp + 1) per lane: one add and a 16-lane DPP reduction per value.  (With one source per lane and 32
  // lanes per combo the two DPP rows had to be joined through v_readlane: 0.29 us of the 2.52 us step with the
  // reduction taken out.)
  // h_{t_prev} loader: lane l < UPW of wave w owns unit UPW w + l (this wave's own dW unit tiles: wave-private LDS rows)
  const bool h_lane = fuse_dw && lane < UPW;
  const int hunit = UPW * wave + (lane < UPW ? lane : 0);
  // Forward data of the pointwise threads (dy, saved gates, c) is fetched TWO steps ahead and always right after a
  // poll has completed: these are HBM first touches (~2 us), vmcnt retires in order, and a load issued shortly before
  // a poll makes that poll wait for it.  c_{t_prev} of step s is c_t of step s + 1: no load of its own.
  float n1_dy = 0.f, n1_ct = 0.f, n2_dy = 0.f, n2_ct = 0.f;
  float4 n1_av = make_float4(0.f, 0.f, 0.f, 0.f), n2_av = make_float4(0.f, 0.f, 0.f, 0.f);
  float n_h[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) n_h[r] = 0.f;
  auto time_of = [&](int sn) { return d == 0 ? T - 1 - sn : sn; };
  auto fetch_step = [&](int sn, float& o_dy, float& o_ct, float4& o_av) {
    const int tt = time_of(sn);
    const int64_t so = ROW_AT(tt) * ldy + d * PH + punit;
    o_dy = a.dy[so];
    o_av = *reinterpret_cast<const float4*>(a.gates + ROW_AT(tt) * ldg + (int64_t)d * 4 * PH + punit * 4);
    o_ct = a.c[so];
  };
  // forward hidden state at the time that fed step sn's time.  Bare loads from clamped addresses: nothing may touch a
  // loaded value here (a select right after the load makes hipcc wait for it on the spot: an HBM round trip on the
  // serial chain); rows / times that do not exist are zeroed when the registers are staged (stage_h).
  // Addressing: one per-lane byte offset (its unit) + a scalar offset per row and step through a buffer resource whose base
  // is the time slab - eight bare buffer loads.  With per-lane 64-bit pointers hipcc spent ~10 VALU instructions (64-bit
  // multiply-adds) in front of every load: 0.23 us of the 2.30 us step (measured against a build without the h prefetch).
  const unsigned h_voff = (unsigned)(d * PH + hunit) * 4u;
  auto fetch_h = [&](int sn) {
    const int tt = time_of(sn);
    const int ttp = d == 0 ? tt - 1 : tt + 1;
    const bool hp = d == 0 ? (tt > 0) : (tt < T - 1);
    const float* slab = a.yfwd + (int64_t)(hp ? ttp : tt) * B * ldy;
    const __amdgpu_buffer_rsrc_t hrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(slab), 0, 0x7ffffff0, 0x00020000);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int row = r0 + r < a.nb ? r0 + r : r0;
      n_h[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(hrs, h_voff, (unsigned)(row * ldy) * 4u, 0));
    }
  };
  auto stage_h = [&](int buf, int sn) {  // n_h (fetched for step sn) -> this lane's unit, slot buf of the h tile
    if constexpr (FUSE) {
      const int tt = time_of(sn);
      const bool hp = d == 0 ? (tt > 0) : (tt < T - 1);
      float hv[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) hv[r] = (hp && r0 + r < a.nb) ? n_h[r] : 0.f;
      unsigned hi[NR / 2], lo[NR / 2];
#pragma unroll
      for (int r = 0; r < NR / 2; ++r) {
        hi[r] = bf3_hi(hv[2 * r]) | (bf3_hi(hv[2 * r + 1]) << 16);
        lo[r] = bf3_lo(hv[2 * r]) | (bf3_lo(hv[2 * r + 1]) << 16);
      }
      if (NR == 8) {
        *reinterpret_cast<u32x4*>(&ht2[0][hunit][buf][0]) = (u32x4){hi[0], hi[1], hi[NR / 2 - 2], hi[NR / 2 - 1]};
        *reinterpret_cast<u32x4*>(&ht2[1][hunit][buf][0]) = (u32x4){lo[0], lo[1], lo[NR / 2 - 2], lo[NR / 2 - 1]};
      } else {
        *reinterpret_cast<uint2*>(&ht2[0][hunit][buf][0]) = make_uint2(hi[0], hi[1]);
        *reinterpret_cast<uint2*>(&ht2[1][hunit][buf][0]) = make_uint2(lo[0], lo[1]);
      }
    }
  };
  // gather descriptors (loop invariant): byte offset of this lane's quads in parity 0, and whether they exist
  unsigned goff[NE];
  const int gcombo = CPW * wave + (rr < CPW ? rr : 0);
  const int grow = gcombo / QPU, guq = gcombo - grow * QPU;
  const bool guse = rr < CPW && grow < NR && r0 + grow < a.nb;
#pragma unroll
  for (int e = 0; e < NE; ++e)
    goff[e] = (unsigned)((xg - reinterpret_cast<float*>(a.xch)) + ((slice * 32 + 2 * sp + e) * PRG + grow) * PUC + 4 * guq) * 4u;
  u32x4 q[NE];
  bool q_inflight = false;            // q holds an attempt issued in the middle of the previous step's dW_hh block
  if (prow_ok) {
    fetch_step(0, n1_dy, n1_ct, n1_av);
    if (T > 1) fetch_step(1, n2_dy, n2_ct, n2_av);
  }
  if (h_lane) fetch_h(0);
  // dW_hh accumulators: D[m = local column 16 ct + 4 (l >> 4) + i][n = unit 16 (MTW wave + ut) + (l & 15)]
  f32x4 dwacc[CT][MTW];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int ut = 0; ut < MTW; ++ut) dwacc[ct][ut] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float4 st_da = make_float4(0.f, 0.f, 0.f, 0.f);
  float4* st_gp = nullptr;
  __syncthreads();                             // LDS zero fill
  if (h_lane) stage_h(0, 0);
  if (h_lane && T > 1) fetch_h(1);
  unsigned abort_seen = 0u;
  for (int s = 0; s < T; ++s) {
    const int t = time_of(s);
    LP_MARK(0);
    // another workgroup's abort: looked at every 16th step only (an agent-scope load and its wait on every step of the
    // chain is not needed: a CU whose producers stopped publishing finds the flag in its spin loop)
    if (ASR_ABORT_PERIOD_MASK == 0 || (s & ASR_ABORT_PERIOD_MASK) == 0) {
      if (pw_thread && flag_load(a.ctrl + 8) != 0u) abort_seen = 1u;
    }
    const float dyv = n1_dy, ct_ = n1_ct;
    const float4 av = n1_av;
    // rotate: n1 <- n2 (step s + 1's).  Opaque moves: left to itself hipcc renames the rotation away and instead copies
    // each prefetched value out of a temporary right after its load - a wait for an HBM round trip on the serial chain.
    asm volatile("v_mov_b32 %0, %1" : "=v"(n1_dy) : "v"(n2_dy));
    asm volatile("v_mov_b32 %0, %1" : "=v"(n1_ct) : "v"(n2_ct));
    asm volatile("v_mov_b32 %0, %1" : "=v"(n1_av.x) : "v"(n2_av.x));
    asm volatile("v_mov_b32 %0, %1" : "=v"(n1_av.y) : "v"(n2_av.y));
    asm volatile("v_mov_b32 %0, %1" : "=v"(n1_av.z) : "v"(n2_av.z));
    asm volatile("v_mov_b32 %0, %1" : "=v"(n1_av.w) : "v"(n2_av.w));
    const float cp = s + 1 < T ? n1_ct : 0.f;                     // c at the time that feeds this one
    // Everything of the pointwise backward that only needs forward data (the tanh, the gate derivatives) is formed HERE,
    // before the gather: after it the chain is dh -> dc -> dG, seven multiply-adds (the compiler left all of it behind
    // barrier A, two transcendentals and ~25 dependent VALU instructions on the serial chain)
    float k_dc = 0.f, k_i = 0.f, k_f = 0.f, k_g = 0.f, k_o = 0.f, k_cn = 0.f;
    if (pw_thread) {
      const float tc = asr_fast_tanh(ct_);
      const bool live = t < plen;
      k_dc = av.w * (1.f - tc * tc);
      k_i = live ? av.z * av.x * (1.f - av.x) : 0.f;
      k_f = live ? cp * av.y * (1.f - av.y) : 0.f;
      k_g = live ? av.x * (1.f - av.z * av.z) : 0.f;
      k_o = live ? tc * av.w * (1.f - av.w) : 0.f;
      k_cn = live ? av.y : 0.f;
      asm volatile("" : "+v"(k_dc), "+v"(k_i), "+v"(k_f), "+v"(k_g), "+v"(k_o), "+v"(k_cn));
    }
    // h tile of the NEXT step (fetched after the previous poll, a whole step ago) -> the other LDS slot, while this step's
    // partials are still in flight.  (Behind the poll instead of here: 2.27 vs 2.16 us per step; a first poll attempt issued
    // before this staging: 2.22 vs 2.14 us - an attempt that arrives before the data costs a second L2 round trip.)
    if (h_lane && s + 1 < T) stage_h((s + 1) & 3, s + 1);
    float4* gp = nullptr;
    if (prow_ok) gp = reinterpret_cast<float4*>(a.gates + ROW_AT(t) * ldg + (int64_t)d * 4 * PH + punit * 4);
    // ---------------------------------------------------------------- (1) gather the partials addressed to this CU
    float dh_rec = 0.f;
    if (s > 0) {
      const unsigned tb = tag_bit_of_step(s - 1);
      unsigned spins = 0;
      while (true) {
        bool ok = true;
        if (!q_inflight) {
#pragma unroll
          for (int e = 0; e < NE; ++e) q[e] = __builtin_amdgcn_raw_buffer_load_b128(xrs, goff[e] + (unsigned)(((s - 1) & 1) * PARSZ) * 4u, 0, 16);
        }
        q_inflight = false;
#pragma unroll
        for (int e = 0; e < NE; ++e) ok = ok && (!guse || quad_ok(q[e], tb));
        if (__all(ok)) break;
        if (++spins > SPIN_LIMIT || ((spins & 63u) == 0u && flag_load(a.ctrl + 8) != 0u)) {
          if (lane == 0) raise_abort(a.ctrl, 3u);
          aborted = true;
          break;
        }
        __builtin_amdgcn_s_sleep(POLL_SLEEP);
      }
      LP_MARK(1);
      float v[4] = {__uint_as_float(q[0].x) + __uint_as_float(q[1].x), __uint_as_float(q[0].y) + __uint_as_float(q[1].y),
                    __uint_as_float(q[0].z) + __uint_as_float(q[1].z), __uint_as_float(q[0].w) + __uint_as_float(q[1].w)};
      row16_sum4(v);                               // every lane of a 16-lane row holds the row's total
      if constexpr (ROWPW) dh_rec = (sp & 2) ? ((sp & 1) ? v[3] : v[2]) : ((sp & 1) ? v[1] : v[0]);
      else if (sp == 0 && guse) *reinterpret_cast<float4*>(&dhs[grow][4 * guq]) = make_float4(v[0], v[1], v[2], v[3]);
    }
    if (st_gp) { // previous step's dG (bulk store after the poll: vmcnt retires in order)
      *st_gp = st_da;
      st_gp = nullptr;
    }
    // prefetches: right after the poll, i.e. as far ahead of the next one as possible
    if (prow_ok && s + 2 < T) fetch_step(s + 2, n2_dy, n2_ct, n2_av);
    if constexpr (FUSE) {
      if (h_lane && s + 2 < T) fetch_h(s + 2);
      LP_MARK(2);
      __syncthreads();                 // A: the h tile / dG slots of the fused dW_hh block (the unfused kernel alternates two
      LP_MARK(3);                      // dG slots instead: a slot is rewritten two barriers B after its last reader)
    }
    // ---------------------------------------------------------------- (2) pointwise LSTM backward of this CU's units
    if (pw_lane) {
      float4 da = make_float4(0.f, 0.f, 0.f, 0.f);
      if (pw_thread) {
        const float dh = dyv + (ROWPW ? dh_rec : (s > 0 ? dhs[pj][pu] : 0.f));
        const float dc = dcarry + dh * k_dc;
        da.x = dc * k_i;
        da.y = dc * k_f;
        da.z = dc * k_g;
        da.w = dh * k_o;
        const float dcn = dc * k_cn;
        if (aborted || abort_seen != 0u) da.x = __builtin_nanf("");
        dcarry = dcn;
        {
          const int sl = FUSE ? (s & 3) : (s & 1), zs = (s + 1) & 3;   // this step's slot; the slot the NEXT step's h is staged into
          unsigned p0[NT], p1[NT];
          bfn_split2<NT>(da.x, da.y, p0);
          bfn_split2<NT>(da.z, da.w, p1);
#pragma unroll
          for (int k = 0; k < NT; ++k) *reinterpret_cast<uint2*>(&dgs[k][sl][pj][4 * pu]) = make_uint2(p0[k], p1[k]);
          if constexpr (FUSE) {
            if (fuse_dw) {              // must read as zero in the flush that does not cover it
#pragma unroll
              for (int k = 0; k < NT; ++k) *reinterpret_cast<uint2*>(&dgs[k][zs][pj][4 * pu]) = make_uint2(0u, 0u);
            }
          }
        }
        if (prow_ok) {
          st_da = da;
          st_gp = (!PACKED || t < pext) ? gp : nullptr;
          dbacc.x += da.x; dbacc.y += da.y; dbacc.z += da.z; dbacc.w += da.w;
        }
      }
    }
    LP_MARK(4);
    __syncthreads();                                                                                     // B
    LP_MARK(5);
    // ---------------------------------------------------------------- (3) partial dh of all units, publish
    {
      f32x4 acc[MTW];
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        if constexpr (NT == 3) {
          // columns 8..15 of the batch side carry a second term (fold_halves): four MFMAs per tile and k-step
          const u32x4 b1 = *reinterpret_cast<const u32x4*>(&dgs[ml >> 3][s & 1][ml & 7][32 * ks + 8 * kq]);
          const u32x4 b2 = *reinterpret_cast<const u32x4*>(&dgs[2 + (ml >> 3)][s & 1][ml & 7][32 * ks + 8 * kq]);
#pragma unroll
          for (int mt = 0; mt < MTW; ++mt) acc[mt] = bf3_mfma(wt[mt][ks][0], b1, acc[mt]);
#pragma unroll
          for (int mt = 0; mt < MTW; ++mt) acc[mt] = bf3_mfma(wt[mt][ks][1], b1, acc[mt]);
#pragma unroll
          for (int mt = 0; mt < MTW; ++mt) acc[mt] = bf3_mfma(wt[mt][ks][0], b2, acc[mt]);
#pragma unroll
          for (int mt = 0; mt < MTW; ++mt) acc[mt] = bf3_mfma(wt[mt][ks][2], b1, acc[mt]);
        } else {
          const u32x4 bh = *reinterpret_cast<const u32x4*>(&dgs[0][s & 3][ml & 7][32 * ks + 8 * kq]);
          const u32x4 bl = *reinterpret_cast<const u32x4*>(&dgs[1][s & 3][ml & 7][32 * ks + 8 * kq]);
#pragma unroll
          for (int mt = 0; mt < MTW; ++mt) acc[mt] = bf3_mfma(wt[mt][ks][0], bh, acc[mt]);
#pragma unroll
          for (int mt = 0; mt < MTW; ++mt) acc[mt] = bf3_mfma(wt[mt][ks][0], bl, acc[mt]);
#pragma unroll
          for (int mt = 0; mt < MTW; ++mt) acc[mt] = bf3_mfma(wt[mt][ks][1], bh, acc[mt]);
        }
      }
      if constexpr (NT == 3) {
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) fold_halves(acc[mt]);
      }
      LP_MARK(6);
      // D: lane l holds units 16 tile + 4 (l >> 4) .. + 3 of batch row l & 15 -> one tagged quad to their owner's slot
      if (ml < NR && s + 1 < T) {
        const unsigned bit = tag_bit_of_step(s);
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) {
          const int ug = 16 * (MTW * wave + mt) + 4 * kq;
          const int dest = ug / PUC, uo = ug - dest * PUC;
          const unsigned doff = (unsigned)((xg - reinterpret_cast<float*>(a.xch)) + (s & 1) * PARSZ +
                                           ((dest * 32 + slice) * PRG + ml) * PUC + uo) * 4u;
          // one 16-byte store (plain: it stays in this XCD's L2); every word carries its own tag, tearing is harmless
          const u32x4 tq = {__float_as_uint(tag_word(acc[mt][0], bit)), __float_as_uint(tag_word(acc[mt][1], bit)),
                            __float_as_uint(tag_word(acc[mt][2], bit)), __float_as_uint(tag_word(acc[mt][3], bit))};
          __builtin_amdgcn_raw_buffer_store_b128(tq, xrs, doff, 0, 0);
        }
      }
    }
    LP_MARK(7);
    // ---------------------------------------------------------------- (4) off the serial chain
    // dW_hh += dG_t^T h_{t_prev} (A = local dG [col][k], B = h [unit][k], k = (slot, row)): once every THREE steps for the
    // three steps just done.  A single step only fills 8 of the K = 32 of the bf16 MFMA and every shape costs the same
    // 16 cycles, so a per-step product was 1 536 MFMA cycles per SIMD and step; the fourth slot is the one the next
    // step's h is being staged into (its dG slot is kept zero), which lets the staging stay where the prefetch needs it.
    if constexpr (FUSE) if (fuse_dw && (s % 3 == 2 || s == T - 1)) {
      if (s % 3 != 2) {
        // tail of the sequence (1 or 2 pending steps): slots of steps that were flushed already must read as zero
        __syncthreads();
        if (pw_thread) {
#pragma unroll
          for (int sl = 0; sl < 4; ++sl) {
            const bool pending = sl == (s & 3) || (s % 3 == 1 && sl == ((s - 1) & 3));
            if (!pending) {
#pragma unroll
              for (int k = 0; k < NT; ++k) *reinterpret_cast<uint2*>(&dgs[k][sl][pj][4 * pu]) = make_uint2(0u, 0u);
            }
          }
        }
        __syncthreads();
      }
      // lane (column 16 ct + ml, slot kq) <- rows 0..7 of that column of slot kq: lane 4 q + p of the 16-lane group
      // supplies the address of row q (second read: row 4 + q), columns 16 ct + 4 p .. + 3
      const int tq = ml >> 2, tp = ml & 3;
      auto a_frag = [&](int k, int ct) -> u32x4 {
        const s16x4 f0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)&dgs[k][kq][tq][16 * ct + 4 * tp]);
        const s16x4 f1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)&dgs[k][kq][4 + tq][16 * ct + 4 * tp]);
        const uint2 u0 = __builtin_bit_cast(uint2, f0), u1 = __builtin_bit_cast(uint2, f1);
        return (u32x4){u0.x, u0.y, u1.x, u1.y};
      };
      auto first_attempt = [&]() {
        // first attempt at the next step's partials, issued half way through this block: the round trip runs under
        // the remaining MFMAs, and the poll at the top of the next step starts by looking at what came back
#pragma unroll
        for (int e = 0; e < NE; ++e) q[e] = __builtin_amdgcn_raw_buffer_load_b128(xrs, goff[e] + (unsigned)((s & 1) * PARSZ) * 4u, 0, 16);
        q_inflight = true;
      };
      if constexpr (FUSE) {
        u32x4 ah[CT], al[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) { ah[ct] = a_frag(0, ct); al[ct] = a_frag(1, ct); }
#pragma unroll
        for (int ut = 0; ut < MTW; ++ut) {
          if (ut == (MTW + 1) / 2 && s + 1 < T) first_attempt();
          const int un = 16 * (MTW * wave + ut) + ml;
          const u32x4 bh = *reinterpret_cast<const u32x4*>(&ht2[0][un][kq][0]);
          const u32x4 bl = *reinterpret_cast<const u32x4*>(&ht2[1][un][kq][0]);
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) dwacc[ct][ut] = bf3_mfma(ah[ct], bh, dwacc[ct][ut]);
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) dwacc[ct][ut] = bf3_mfma(ah[ct], bl, dwacc[ct][ut]);
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) dwacc[ct][ut] = bf3_mfma(al[ct], bh, dwacc[ct][ut]);
        }
      }
      LP_MARK(8);
    }
  }
  // an abort raised by another workgroup during the last steps (inside the loop the flag is sampled every 16th step only):
  // this CU's partial sums were incomplete then, so its last dG row and its weight / bias gradients are poisoned as well
  if (flag_load(a.ctrl + 8) != 0u) {
    st_da.x = __builtin_nanf("");
    dbacc.x = __builtin_nanf("");
    dwacc[0][0][0] = __builtin_nanf("");
  }
  if (st_gp) *st_gp = st_da;
  // packed rows: dG of the block's padding rows behind the T steps that were run (PersistArgs)
  if constexpr (PACKED) if (prow_ok) {
    for (int tt = T; tt < pext; ++tt)
      *reinterpret_cast<float4*>(a.gates + ROW_AT(tt) * ldg + (int64_t)d * 4 * PH + punit * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (a.db != nullptr) {        // one atomic per (unit, gate) and CU; the rows are summed through LDS
    if (pw_lane) *reinterpret_cast<float4*>(&dbs[pj][4 * pu]) = dbacc;
    __syncthreads();
    if (tid < 4 * PUR) {
      float v = 0.f;
#pragma unroll
      for (int r = 0; r < PRG; ++r) v += dbs[r][tid];
      atomicAdd(a.db + (int64_t)d * 4 * PH + PUR * slice * 4 + tid, v);
    }
  }
  if (fuse_dw) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int ut = 0; ut < MTW; ++ut)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int col = 16 * ct + 4 * kq + i, un = 16 * (MTW * wave + ut) + ml;
          if (col < NC) atomicAdd(a.dw + ((int64_t)d * 4 * PH + NC * slice + col) * PH + un, dwacc[ct][ut][i]);
        }
  }
}

// ------------------------------------------------------ backward, exchanged partials, H = 640 (the judge LM's width)
// lstm_persist_bwd_rs_kernel's unfused three-term form for 20 units per CU, which its layout does not reach:
//   * 80 local gate columns = two k-steps of 32 plus ONE OF 16 on v_mfma_f32_16x16x16_bf16 (three full k-steps would be 180
//     weight registers; this is 150), 40 unit tiles = 5 per wave;
//   * 5 unit quads per row: DPP rows 0..3 of wave w gather quads 0..3 of row w as there, and row 0 gathers quad 4 on top
//     (two more quads for its 16 lanes);
//   * pointwise lanes: lanes 0..3 of DPP row rr -> unit 4 rr + lane, lanes 4..7 of row 0 -> units 16..19.
// Everything else (exchange layout [dest][src][row][unit], tags, abort handling, stores / prefetches behind the poll, two
// dG slots, forward-data factors formed in front of the gather) is that kernel's.  dW_hh is left to the caller, db is summed.
template <int NR, bool PACKED = false>
__global__ __launch_bounds__(PNT) void lstm_persist_bwd_rs640_kernel(PersistArgs a) {
  constexpr int PH = 640, NT = 3, PUC = 20, NC = 80, MTW = 5, GST = 96 + 8, NE = 2;
  constexpr int PARSZ = 32 * 32 * PRG * PUC;      // floats per parity
  __shared__ __attribute__((aligned(16))) unsigned short dgs[4][2][PRG][GST];   // terms a, b, c + a zero image; two slots
  __shared__ __attribute__((aligned(16))) float dbs[PRG][4 * PUC];
  __shared__ int role[2];
  extern __shared__ float occupancy_pad[];                                // forces one workgroup per CU
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i < 4 * 2 * PRG * GST; i += PNT) (&dgs[0][0][0][0])[i] = 0;
  for (int i = tid; i < PRG * 4 * PUC; i += PNT) (&dbs[0][0])[i] = 0.f;
  int g, slice;
  take_role(a.ctrl, role, g, slice);
  if (slice < 0) return;
  const int T = a.T, B = a.B, ndir = a.ndir;
  const int d = ndir == 2 ? (g & 1) : 0;
  const int rowgroup = ndir == 2 ? (g >> 1) : g;
  const int r0 = rowgroup * NR;
  if (r0 >= a.nb) return;
  const int64_t ldy = (int64_t)ndir * PH, ldg = (int64_t)ndir * 4 * PH;
  const int ml = lane & 15, kq = lane >> 4;
  // W_hh rows of this CU's 80 columns, all 640 units -> split bf16: lane l holds unit 16 (5 wave + mt) + (l & 15);
  // full k-steps: columns 32 ks + 8 (l >> 4) + j, tail: columns 64 + 4 (l >> 4) + j
  u32x4 wt[MTW][2][NT];
  uint2 wtl[MTW][NT];
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt) {
    const int cu = 16 * (MTW * wave + mt) + ml;
    auto wel = [&](int k) -> float {
      return a.w_il != nullptr ? a.w_il[((int64_t)d * 4 * PH + NC * slice + k) * PH + cu]
                               : a.w[((int64_t)d * PH + cu) * (4 * PH) + NC * slice + k];
    };
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = wel(32 * ks + 8 * kq + j);
      bfn_split8<NT>(v, wt[mt][ks]);
    }
    unsigned p0[NT], p1[NT];
    bfn_split2<NT>(wel(64 + 4 * kq), wel(64 + 4 * kq + 1), p0);
    bfn_split2<NT>(wel(64 + 4 * kq + 2), wel(64 + 4 * kq + 3), p1);
#pragma unroll
    for (int k = 0; k < NT; ++k) wtl[mt][k] = make_uint2(p0[k], p1[k]);
  }
  const int rr = lane >> 4, sp = lane & 15;
  const int pu = sp < 4 ? 4 * rr + sp : 16 + (sp & 3), pj = wave;
  const bool pw_lane = sp < 4 || (rr == 0 && sp < 8);
  const bool pw_thread = pw_lane && pj < NR;
  const int prow = r0 + pj;
  const bool prow_ok = pw_thread && prow < a.nb;
  const int punit = PUC * slice + pu;
  const int plen = prow_ok ? a.lens[prow] : 0;
  // Row of (time, this thread's batch row); see PersistArgs.  PACKED is a template parameter, not a run-time branch: the
  // time-major instantiation must compile from the expression it was tuned with.  These kernels live on the register
  // allocator's goodwill - the forward data of a step is prefetched two steps ahead, and an allocation that cannot give a
  // 16-byte load the four registers its value stays in copies it out of a temporary RIGHT BEHIND the load: a wait for an
  // HBM first touch on the serial chain (bwd 1.80 -> 2.30 us per time step when the run-time form of this map moved it).
  // tools/isa_waits.py lists the vmcnt waits of a kernel's loop; none may follow the prefetch loads.
  const int pbase = (PACKED && prow_ok) ? a.rowbase[prow] : 0;
  const int pext = PACKED ? (prow_ok ? a.rowext[prow] : 1) : a.T;
  // (ROW_AT is a macro, not a lambda: with by-reference captures in the way hipcc allocated the backward kernel's
  // registers differently - see above)
  float dcarry = 0.f;
  float4 dbacc = make_float4(0.f, 0.f, 0.f, 0.f);
  float* xg = reinterpret_cast<float*>(a.xch) + (int64_t)g * (2 * PARSZ);
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(a.xch, 0, 0x7ffffff0, 0x00020000);
  bool aborted = false;
  float n1_dy = 0.f, n1_ct = 0.f, n2_dy = 0.f, n2_ct = 0.f;
  float4 n1_av = make_float4(0.f, 0.f, 0.f, 0.f), n2_av = make_float4(0.f, 0.f, 0.f, 0.f);
  auto time_of = [&](int sn) { return d == 0 ? T - 1 - sn : sn; };
  auto fetch_step = [&](int sn, float& o_dy, float& o_ct, float4& o_av) {
    const int tt = time_of(sn);
    const int64_t so = ROW_AT(tt) * ldy + d * PH + punit;
    o_dy = a.dy[so];
    o_av = *reinterpret_cast<const float4*>(a.gates + ROW_AT(tt) * ldg + (int64_t)d * 4 * PH + punit * 4);
    o_ct = a.c[so];
  };
  // gather descriptors: DPP row rr sums the 32 sources of (row = wave, unit quad rr), two sources per lane; row 0 also quad 4
  const bool guse = wave < NR && r0 + wave < a.nb;
  unsigned goff[NE], goff4[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const unsigned base = (unsigned)((xg - reinterpret_cast<float*>(a.xch)) + ((slice * 32 + 2 * sp + e) * PRG + (guse ? wave : 0)) * PUC);
    goff[e] = (base + 4 * rr) * 4u;
    goff4[e] = (base + 16) * 4u;
  }
  u32x4 q[NE], q4[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) q4[e] = (u32x4){0u, 0u, 0u, 0u};
  if (prow_ok) {
    fetch_step(0, n1_dy, n1_ct, n1_av);
    if (T > 1) fetch_step(1, n2_dy, n2_ct, n2_av);
  }
  float4 st_da = make_float4(0.f, 0.f, 0.f, 0.f);
  float4* st_gp = nullptr;
  __syncthreads();                             // LDS zero fill
  unsigned abort_seen = 0u;
  for (int s = 0; s < T; ++s) {
    const int t = time_of(s);
    if (ASR_ABORT_PERIOD_MASK == 0 || (s & ASR_ABORT_PERIOD_MASK) == 0) {
      if (pw_thread && flag_load(a.ctrl + 8) != 0u) abort_seen = 1u;
    }
    const float dyv = n1_dy, ct_ = n1_ct;
    const float4 av = n1_av;
    asm volatile("v_mov_b32 %0, %1" : "=v"(n1_dy) : "v"(n2_dy));
    asm volatile("v_mov_b32 %0, %1" : "=v"(n1_ct) : "v"(n2_ct));
    asm volatile("v_mov_b32 %0, %1" : "=v"(n1_av.x) : "v"(n2_av.x));
    asm volatile("v_mov_b32 %0, %1" : "=v"(n1_av.y) : "v"(n2_av.y));
    asm volatile("v_mov_b32 %0, %1" : "=v"(n1_av.z) : "v"(n2_av.z));
    asm volatile("v_mov_b32 %0, %1" : "=v"(n1_av.w) : "v"(n2_av.w));
    const float cp = s + 1 < T ? n1_ct : 0.f;                     // c at the time that feeds this one
    // forward-data factors of the pointwise backward: in front of the gather (see lstm_persist_bwd_rs_kernel)
    float k_dc = 0.f, k_i = 0.f, k_f = 0.f, k_g = 0.f, k_o = 0.f, k_cn = 0.f;
    if (pw_thread) {
      const float tc = asr_fast_tanh(ct_);
      const bool live = t < plen;
      k_dc = av.w * (1.f - tc * tc);
      k_i = live ? av.z * av.x * (1.f - av.x) : 0.f;
      k_f = live ? cp * av.y * (1.f - av.y) : 0.f;
      k_g = live ? av.x * (1.f - av.z * av.z) : 0.f;
      k_o = live ? tc * av.w * (1.f - av.w) : 0.f;
      k_cn = live ? av.y : 0.f;
      asm volatile("" : "+v"(k_dc), "+v"(k_i), "+v"(k_f), "+v"(k_g), "+v"(k_o), "+v"(k_cn));
    }
    float4* gp = nullptr;
    if (prow_ok) gp = reinterpret_cast<float4*>(a.gates + ROW_AT(t) * ldg + (int64_t)d * 4 * PH + punit * 4);
    // ---------------------------------------------------------------- (1) gather the partials addressed to this CU
    float dh_rec = 0.f;
    if (s > 0) {
      const unsigned tb = tag_bit_of_step(s - 1);
      const unsigned par = (unsigned)(((s - 1) & 1) * PARSZ) * 4u;
      unsigned spins = 0;
      while (true) {
        bool ok = true;
#pragma unroll
        for (int e = 0; e < NE; ++e) q[e] = __builtin_amdgcn_raw_buffer_load_b128(xrs, goff[e] + par, 0, 16);
        if (rr == 0) {
#pragma unroll
          for (int e = 0; e < NE; ++e) q4[e] = __builtin_amdgcn_raw_buffer_load_b128(xrs, goff4[e] + par, 0, 16);
        }
#pragma unroll
        for (int e = 0; e < NE; ++e) ok = ok && (!guse || (quad_ok(q[e], tb) && (rr != 0 || quad_ok(q4[e], tb))));
        if (__all(ok)) break;
        if (++spins > SPIN_LIMIT || ((spins & 63u) == 0u && flag_load(a.ctrl + 8) != 0u)) {
          if (lane == 0) raise_abort(a.ctrl, 3u);
          aborted = true;
          break;
        }
        __builtin_amdgcn_s_sleep(POLL_SLEEP);
      }
      float v[4] = {__uint_as_float(q[0].x) + __uint_as_float(q[1].x), __uint_as_float(q[0].y) + __uint_as_float(q[1].y),
                    __uint_as_float(q[0].z) + __uint_as_float(q[1].z), __uint_as_float(q[0].w) + __uint_as_float(q[1].w)};
      float v4[4] = {__uint_as_float(q4[0].x) + __uint_as_float(q4[1].x), __uint_as_float(q4[0].y) + __uint_as_float(q4[1].y),
                     __uint_as_float(q4[0].z) + __uint_as_float(q4[1].z), __uint_as_float(q4[0].w) + __uint_as_float(q4[1].w)};
      row16_sum4(v);                               // every lane of a 16-lane row holds the row's totals
      row16_sum4(v4);                              // (meaningful in DPP row 0 only)
      const float pa = (sp & 2) ? ((sp & 1) ? v[3] : v[2]) : ((sp & 1) ? v[1] : v[0]);
      const float pb = (sp & 2) ? ((sp & 1) ? v4[3] : v4[2]) : ((sp & 1) ? v4[1] : v4[0]);
      dh_rec = sp < 4 ? pa : pb;
    }
    if (st_gp) {                                  // previous step's dG (bulk store after the poll: vmcnt retires in order)
      *st_gp = st_da;
      st_gp = nullptr;
    }
    if (prow_ok && s + 2 < T) fetch_step(s + 2, n2_dy, n2_ct, n2_av);
    // ---------------------------------------------------------------- (2) pointwise LSTM backward in the gather lanes
    if (pw_thread) {
      const float dh = dyv + dh_rec;
      const float dc = dcarry + dh * k_dc;
      float4 da = make_float4(dc * k_i, dc * k_f, dc * k_g, dh * k_o);
      if (aborted || abort_seen != 0u) da.x = __builtin_nanf("");
      dcarry = dc * k_cn;
      unsigned p0[NT], p1[NT];
      bfn_split2<NT>(da.x, da.y, p0);
      bfn_split2<NT>(da.z, da.w, p1);
#pragma unroll
      for (int k = 0; k < NT; ++k) *reinterpret_cast<uint2*>(&dgs[k][s & 1][pj][4 * pu]) = make_uint2(p0[k], p1[k]);
      if (prow_ok) {
        st_da = da;
        st_gp = (!PACKED || t < pext) ? gp : nullptr;
        dbacc.x += da.x; dbacc.y += da.y; dbacc.z += da.z; dbacc.w += da.w;
      }
    }
    __syncthreads();                                                                                     // B
    // ---------------------------------------------------------------- (3) partial dh of all units, publish
    {
      f32x4 acc[MTW];
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        // columns 8..15 of the batch side carry a second term (fold_halves): four MFMAs per tile and k-step
        const u32x4 b1 = *reinterpret_cast<const u32x4*>(&dgs[ml >> 3][s & 1][ml & 7][32 * ks + 8 * kq]);
        const u32x4 b2 = *reinterpret_cast<const u32x4*>(&dgs[2 + (ml >> 3)][s & 1][ml & 7][32 * ks + 8 * kq]);
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) acc[mt] = bf3_mfma(wt[mt][ks][0], b1, acc[mt]);
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) acc[mt] = bf3_mfma(wt[mt][ks][1], b1, acc[mt]);
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) acc[mt] = bf3_mfma(wt[mt][ks][0], b2, acc[mt]);
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) acc[mt] = bf3_mfma(wt[mt][ks][2], b1, acc[mt]);
      }
      {
        const uint2 b1 = *reinterpret_cast<const uint2*>(&dgs[ml >> 3][s & 1][ml & 7][64 + 4 * kq]);
        const uint2 b2 = *reinterpret_cast<const uint2*>(&dgs[2 + (ml >> 3)][s & 1][ml & 7][64 + 4 * kq]);
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) acc[mt] = bf3_mfma16(wtl[mt][0], b1, acc[mt]);
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) acc[mt] = bf3_mfma16(wtl[mt][1], b1, acc[mt]);
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) acc[mt] = bf3_mfma16(wtl[mt][0], b2, acc[mt]);
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) acc[mt] = bf3_mfma16(wtl[mt][2], b1, acc[mt]);
      }
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt) fold_halves(acc[mt]);
      // D: lane l holds units 16 tile + 4 (l >> 4) .. + 3 of batch row l & 15 -> one tagged quad to their owner's slot
      if (ml < NR && s + 1 < T) {
        const unsigned bit = tag_bit_of_step(s);
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) {
          const int ug = 16 * (MTW * wave + mt) + 4 * kq;
          const int dest = ug / PUC, uo = ug - dest * PUC;
          const unsigned doff = (unsigned)((xg - reinterpret_cast<float*>(a.xch)) + (s & 1) * PARSZ +
                                           ((dest * 32 + slice) * PRG + ml) * PUC + uo) * 4u;
          const u32x4 tq = {__float_as_uint(tag_word(acc[mt][0], bit)), __float_as_uint(tag_word(acc[mt][1], bit)),
                            __float_as_uint(tag_word(acc[mt][2], bit)), __float_as_uint(tag_word(acc[mt][3], bit))};
          __builtin_amdgcn_raw_buffer_store_b128(tq, xrs, doff, 0, 0);
        }
      }
    }
  }
  // an abort raised by another workgroup during the last steps (the flag is sampled every 16th step inside the loop)
  if (flag_load(a.ctrl + 8) != 0u) {
    st_da.x = __builtin_nanf("");
    dbacc.x = __builtin_nanf("");
  }
  if (st_gp) *st_gp = st_da;
  // packed rows: dG of the block's padding rows behind the T steps that were run (PersistArgs)
  if constexpr (PACKED) if (prow_ok) {
    for (int tt = T; tt < pext; ++tt)
      *reinterpret_cast<float4*>(a.gates + ROW_AT(tt) * ldg + (int64_t)d * 4 * PH + punit * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (a.db != nullptr) {        // one atomic per (unit, gate) and CU; the rows are summed through LDS
    if (pw_lane) *reinterpret_cast<float4*>(&dbs[pj][4 * pu]) = dbacc;
    __syncthreads();
    if (tid < 4 * PUC) {
      float v = 0.f;
#pragma unroll
      for (int r = 0; r < PRG; ++r) v += dbs[r][tid];
      atomicAdd(a.db + (int64_t)d * 4 * PH + PUC * slice * 4 + tid, v);
    }
  }
}

}  // namespace

namespace {

// Dynamic LDS that keeps a second workgroup off the CU (160 KB): static + pad > 80 KB, so the 256 workgroups of a launch
// are co-resident, one per CU.  The static size is the compiled kernel's own; -1 when it cannot be read.
int one_per_cu_pad(const void* kernel) {
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, kernel) != hipSuccess) return -1;
  const size_t stat = fa.sharedSizeBytes;
  return stat < 82 * 1024 ? (int)(82 * 1024 - stat) : 0;
}

// Launch of a persistent kernel, 256 workgroups x PNT threads: its PACKED instantiation when the arguments carry a row
// map (PersistArgs), its time-major one otherwise.
template <auto TIME_MAJOR, auto PACKED_ROWS>
int launch_persist(const PersistArgs& a, hipStream_t stream) {
  static const int pads[2] = {one_per_cu_pad((const void*)TIME_MAJOR), one_per_cu_pad((const void*)PACKED_ROWS)};
  const auto kernel = a.rowbase ? PACKED_ROWS : TIME_MAJOR;
  const int pad = pads[a.rowbase ? 1 : 0];
  if (pad < 0) return (int)hipErrorInvalidDeviceFunction;
  hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, pad);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(kernel, dim3(256), dim3(PNT), pad, stream, a);
  return 0;
}

// Runtime H -> compile-time width: f(std::integral_constant<int, H>) for H among WIDTHS, ASR_E_SHAPE for any other
template <int... WIDTHS, class F>
int with_width(int H, F&& f) {
  int rc = ASR_E_SHAPE;
  (void)((H == WIDTHS && (rc = f(std::integral_constant<int, WIDTHS>{}), true)) || ...);
  return rc;
}

bool persist_supported(int H) { return H == 128 || H == 256 || H == 320 || H == 512; }
// exchanged-partials backward: H with a multiple of 4 units per CU; H = 320 (10 units per CU in 12 slots) in the unfused
// three-term kernel only
bool rs_supported(int H, int arith) {
  return H == 128 || H == 256 || H == 512 || ((H == 320 || H == 640) && (arith & ASR_ARITH_MASK) == ASR_ARITH_BF16X6);
}
// H = 640 (the judge LM): forward on the bf16 kernels, backward on lstm_persist_bwd_rs640_kernel (three terms) only
bool bwd_persist_width(int H) { return persist_supported(H) || H == 640; }
int rs_slots_per_cu(int H) { return (H / 32 + 3) / 4 * 4; }

// rows per XCD group: 4 when the whole batch fits 4-row groups (half the MFMA work and gather per step), else 8
int forced_rows() {
  static const int forced = [] { const char* e = getenv("ASR_LSTM_ROWS"); return e ? atoi(e) : 0; }();   // measurement
  return forced;
}
int rows_per_group(int nb, int ndir) {
  const int forced = forced_rows();
  if (forced == 4 || forced == PRG) return forced;
  return nb <= 4 * (8 / ndir) ? 4 : PRG;
}
// 16-row groups (forward, H = 512, split-bf16 arithmetics): a row block that fills all eight XCDs with 16 rows each (64 rows
// of a bidirectional layer) takes one traversal of the chain instead of two.  ASR_LSTM_ROWS=16 forces them for any block,
// ASR_LSTM_ROWS=8 / 4 switches them off (measurement, tests).
bool fwd_rows16(int left, int ndir, int H, int arith) {
  if (H != 512 || (arith & ASR_ARITH_MASK) == ASR_ARITH_F32) return false;
  const int forced = forced_rows();
  if (forced == 16) return true;
  return forced == 0 && left >= 16 * (8 / ndir);
}

// arith (include/asr_hip.h): ASR_ARITH_F32 -> the 4x4x1 fp32-MFMA kernels; ASR_ARITH_BF16X6 / _BF16X3 -> the bf16-MFMA
// kernels with three / two split terms.  H = 640 (the judge's width) exists on the bf16 kernels only.
template <int NR, int NT, int RG = PRG>
int dispatch_fwd_split(int H, const PersistArgs& a, hipStream_t stream, bool fault) {
  if (fault) {      // the FAULT instantiations exist for the default arithmetic at H = 512 only
    if constexpr (NT == 3 && RG == PRG)
      if (H == 512)
        return launch_persist<lstm_persist_fwd_bf3_kernel<512, NR, 3, RG, false, true>,
                              lstm_persist_fwd_bf3_kernel<512, NR, 3, RG, true, true>>(a, stream);
    return ASR_E_SHAPE;
  }
  auto launch = [&](auto w) {
    constexpr int PH = decltype(w)::value;
    return launch_persist<lstm_persist_fwd_bf3_kernel<PH, NR, NT, RG, false>, lstm_persist_fwd_bf3_kernel<PH, NR, NT, RG, true>>(a, stream);
  };
  if constexpr (RG == 16) return with_width<512>(H, launch);
  else return with_width<128, 256, 320, 512, 640>(H, launch);
}
template <int NR>
int dispatch_fwd(int H, int arith, const PersistArgs& a, hipStream_t stream) {
  const int ar = arith & ASR_ARITH_MASK;
  const bool fault = (arith & ASR_DEBUG_FAULT) != 0;
  if (ar == ASR_ARITH_BF16X6) return dispatch_fwd_split<NR, 3>(H, a, stream, fault);
  if (fault) return ASR_E_SHAPE;
  if (ar == ASR_ARITH_BF16X3) return dispatch_fwd_split<NR, 2>(H, a, stream, false);
  return with_width<128, 256, 320, 512>(H, [&](auto w) {
    constexpr int PH = decltype(w)::value;
    return launch_persist<lstm_persist_fwd_kernel<PH, NR, false>, lstm_persist_fwd_kernel<PH, NR, true>>(a, stream);
  });
}
// which backward kernel a call takes: 0 gathered-dG with fp32 operands, 1 gathered-dG with split operands, 2 split
// exchanged partials, -1 none
int bwd_kernel_kind(int H, int arith) {
  const int ar = arith & ASR_ARITH_MASK;
  if (H == 640) return (ar == ASR_ARITH_BF16X6 && !(arith & ASR_LSTM_BWD_GATHER)) ? 2 : -1;
  if (ar == ASR_ARITH_F32) return 0;
  if (rs_supported(H, arith) && !(arith & ASR_LSTM_BWD_GATHER)) return 2;
  // the gathered-dG kernel with three terms needs 171 KB of LDS at H = 512
  if (ar == ASR_ARITH_BF16X6 && H > 320) return -1;
  return 1;
}
// NT: terms of the operand split (1: the fp32 operands of kind 0)
template <int NR, int NT>
int dispatch_bwd_terms(int H, int kind, const PersistArgs& a, hipStream_t stream) {
  auto gathered = [&](auto w) {
    constexpr int PH = decltype(w)::value;
    return launch_persist<lstm_persist_bwd_kernel<PH, NR, NT, false>, lstm_persist_bwd_kernel<PH, NR, NT, true>>(a, stream);
  };
  if constexpr (NT == 1) {
    return with_width<128, 256, 320, 512>(H, gathered);
  } else {
    auto exchanged = [&](auto w) {
      constexpr int PH = decltype(w)::value;
      if constexpr (PH == 640)
        return launch_persist<lstm_persist_bwd_rs640_kernel<NR, false>, lstm_persist_bwd_rs640_kernel<NR, true>>(a, stream);
      else
        return launch_persist<lstm_persist_bwd_rs_kernel<PH, NR, NT, false>, lstm_persist_bwd_rs_kernel<PH, NR, NT, true>>(a, stream);
    };
    if constexpr (NT == 3) return kind == 2 ? with_width<128, 256, 320, 512, 640>(H, exchanged) : with_width<128, 256, 320>(H, gathered);
    else return kind == 2 ? with_width<128, 256, 512>(H, exchanged) : with_width<128, 256, 320, 512>(H, gathered);
  }
}
template <int NR>
int dispatch_bwd(int H, int arith, const PersistArgs& a, hipStream_t stream) {
  const int kind = bwd_kernel_kind(H, arith);
  if (kind < 0) return ASR_E_SHAPE;
  if (kind == 0) return dispatch_bwd_terms<NR, 1>(H, kind, a, stream);
  return (arith & ASR_ARITH_MASK) == ASR_ARITH_BF16X6 ? dispatch_bwd_terms<NR, 3>(H, kind, a, stream)
                                                     : dispatch_bwd_terms<NR, 2>(H, kind, a, stream);
}

}  // namespace

// The role assignment needs 8 XCDs x 32 CUs, one workgroup per CU (MI355X); anything else takes the per-step path.
bool asr_persist_device_ok() {
  static int cached = -1;
  if (cached < 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      return false;
    cached = cus == 256 ? 1 : 0;
  }
  return cached == 1;
}

// 1 when asr_lstm_seq_bwd_persist* with these arguments accumulates dW_hh inside the kernel (given y and dw_hh), 0 when the
// caller has to form it (the three-term exchanged-partials kernel: see lstm_persist_bwd_rs_kernel), -1 when no persistent
// backward kernel applies.  The bias gradient is accumulated by every persistent backward kernel.
extern "C" int asr_lstm_bwd_persist_fuses_dw(int H, int arith) {
  if (!bwd_persist_width(H)) return -1;
  const int kind = bwd_kernel_kind(H, arith);
  if (kind < 0) return -1;
  return (kind == 2 && (arith & ASR_ARITH_MASK) == ASR_ARITH_BF16X6) ? 0 : 1;
}

static bool arith_ok(int arith) {
  const int ar = arith & ASR_ARITH_MASK;
  return ar == ASR_ARITH_F32 || ar == ASR_ARITH_BF16X6 || ar == ASR_ARITH_BF16X3;
}

// Returns ASR_E_SHAPE when the fast path does not apply (caller falls back to asr_lstm_seq_fwd).  Batches larger
// than 8 * (8 / ndir) rows run as consecutive launches over row blocks (rows are independent; any batch size: a
// single-GPU batch of 256 is 8 launches per layer).
// xch / ctrl: at least asr_persist_scratch_bytes() (10 MB: the H = 640 backward's exchanged partials; 128 B: persist.h, 16
// latch words + 16 per-launch words; the per-launch words and the exchange area are zeroed here on the stream before every
// launch).
extern "C" int asr_persist_scratch_bytes(int64_t* xch_bytes, int64_t* ctrl_bytes) {
  if (xch_bytes) *xch_bytes = (int64_t)8 * 2 * 32 * 32 * 8 * 20 * 4;     // [8 groups][2 parities][32 dest][32 src][8 rows][20 units] floats
  if (ctrl_bytes) *ctrl_bytes = 128;
  return 0;
}
// Steps a row block of PACKED rows has to run: the largest length of its rows when the caller gave a host copy of lens (the
// kernels zero the padding rows of a block behind the steps they ran), else T.
static int block_steps(int T, const int32_t* lens_host, int rb, int rows) {
  if (!lens_host) return T;
  int m = 1;
  for (int r = 0; r < rows; ++r) m = lens_host[rb + r] > m ? lens_host[rb + r] : m;
  return m < T ? m : T;
}

extern "C" int asr_lstm_seq_fwd_persist(int T, int B, int nb, int H, int ndir, float* gates, const float* w_hh,
                                        const int32_t* lens, const int32_t* rowbase, const int32_t* rowext,
                                        const int32_t* lens_host, float* y, float* c, void* xch, void* ctrl, int arith,
                                        asr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!gates || !w_hh || !lens || !y || !c || !xch || !ctrl || T <= 0 || B <= 0 || nb <= 0 || nb > B || !arith_ok(arith)) return ASR_E_ARG;
  if ((rowbase == nullptr) != (rowext == nullptr) || (lens_host && !rowbase)) return ASR_E_ARG;
  // H = 640 (the judge LM, config.yaml dis_hidden_dim): forward only - 20 units per CU = 5 M tiles of the bf16 MFMA
  if (!(persist_supported(H) || H == 640) || (ndir != 1 && ndir != 2) || !asr_persist_device_ok()) return ASR_E_SHAPE;
  if (H == 640 && (arith & ASR_ARITH_MASK) == ASR_ARITH_F32) return ASR_E_SHAPE;
  const int nr8 = rows_per_group(nb, ndir);
  for (int rb = 0; rb < nb;) {
    const int nr = fwd_rows16(nb - rb, ndir, H, arith) ? 16 : nr8;
    const int rows_per_launch = nr * (8 / ndir);
    hipError_t e = persist_reset(xch, ctrl, (size_t)2 * 8 * (nr > PRG ? nr : PRG) * H * sizeof(u64), stream);
    if (e != hipSuccess) return (int)e;
    PersistArgs a = {};
    a.B = B; a.nb = nb - rb < rows_per_launch ? nb - rb : rows_per_launch; a.ndir = ndir;
    a.T = block_steps(T, lens_host, rb, a.nb);
    // time-major: the row block starts rb rows into every time slab; packed rows: rowbase is absolute
    const int64_t ro = rowbase ? 0 : rb;
    a.gates = gates + ro * ndir * 4 * H; a.w = w_hh; a.lens = lens + rb;
    a.rowbase = rowbase ? rowbase + rb : nullptr; a.rowext = rowext ? rowext + rb : nullptr;
    a.y = y + ro * ndir * H; a.c = c + ro * ndir * H;
    a.dy = nullptr; a.yfwd = nullptr; a.dw = nullptr; a.db = nullptr; a.xch = (u64*)xch; a.ctrl = persist_launch_words(ctrl);
    int rc;
    if (nr == 16)
      rc = (arith & ASR_ARITH_MASK) == ASR_ARITH_BF16X6 ? dispatch_fwd_split<16, 3, 16>(H, a, stream, false)
                                                        : dispatch_fwd_split<16, 2, 16>(H, a, stream, false);
    else
      rc = nr == 4 ? dispatch_fwd<4>(H, arith, a, stream) : dispatch_fwd<PRG>(H, arith, a, stream);
    if (rc) return rc;
    rb += rows_per_launch;
  }
  ASR_CHECK_LAUNCH();
  return 0;
}

// Persistent fast path of asr_lstm_seq_bwd (same arguments and results except that no dcarry scratch is needed).
static int lstm_seq_bwd_persist_impl(int T, int B, int nb, int H, int ndir, float* gates, const float* w_hhT, const float* w_hh_il,
                                     const int32_t* lens, const int32_t* rowbase, const int32_t* rowext,
                                     const int32_t* lens_host, const float* dy, const float* c, const float* y,
                                     float* dw_hh, float* db, void* xch, void* ctrl, int arith, asr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!gates || (!w_hhT && !w_hh_il) || !lens || !dy || !c || !xch || !ctrl || T <= 0 || B <= 0 || nb <= 0 || nb > B || !arith_ok(arith)) return ASR_E_ARG;
  if ((rowbase == nullptr) != (rowext == nullptr) || (lens_host && !rowbase)) return ASR_E_ARG;
  if (rowbase) { y = nullptr; dw_hh = nullptr; }     // packed rows: dW_hh is the caller's (one product over all rows, see asr_hip.h)
  if (!bwd_persist_width(H) || (ndir != 1 && ndir != 2) || !asr_persist_device_ok()) return ASR_E_SHAPE;
  const int kind = bwd_kernel_kind(H, arith);
  if (kind < 0) return ASR_E_SHAPE;
  // the forward-layout weights are only read by the exchanged-partials kernel
  if (!w_hhT && kind != 2) return ASR_E_SHAPE;
  const int nr = rows_per_group(nb, ndir);
  const int rows_per_launch = nr * (8 / ndir);
  for (int rb = 0; rb < nb; rb += rows_per_launch) {
    // exchanged-partials kernel: [8 groups][2 parities][32 dest][32 src][8 rows][H/32 units] floats (8 MB at H = 512)
    const size_t xbytes = kind == 2 ? (size_t)8 * 2 * 32 * 32 * PRG * rs_slots_per_cu(H) * sizeof(float)
                                    : (size_t)2 * 8 * PRG * 4 * H * sizeof(float);
    hipError_t e = persist_reset(xch, ctrl, xbytes, stream);
    if (e != hipSuccess) return (int)e;
    PersistArgs a = {};
    a.B = B; a.nb = nb - rb < rows_per_launch ? nb - rb : rows_per_launch; a.ndir = ndir;
    a.T = block_steps(T, lens_host, rb, a.nb);
    const int64_t ro = rowbase ? 0 : rb;
    a.gates = gates + ro * ndir * 4 * H; a.w = w_hhT; a.w_il = w_hhT ? nullptr : w_hh_il; a.lens = lens + rb; a.y = nullptr;
    a.rowbase = rowbase ? rowbase + rb : nullptr; a.rowext = rowext ? rowext + rb : nullptr;
    a.c = const_cast<float*>(c) + ro * ndir * H; a.dy = dy + ro * ndir * H;
    a.yfwd = (y && dw_hh) ? y + ro * ndir * H : nullptr; a.dw = (y && dw_hh) ? dw_hh : nullptr;
    a.db = db;
    a.xch = (u64*)xch; a.ctrl = persist_launch_words(ctrl);
    int rc = nr == 4 ? dispatch_bwd<4>(H, arith, a, stream) : dispatch_bwd<PRG>(H, arith, a, stream);
    if (rc) return rc;
  }
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_lstm_seq_bwd_persist(int T, int B, int nb, int H, int ndir, float* gates, const float* w_hhT,
                                        const int32_t* lens, const int32_t* rowbase, const int32_t* rowext,
                                        const int32_t* lens_host, const float* dy, const float* c, const float* y,
                                        float* dw_hh, float* db, void* xch, void* ctrl, int arith, asr_stream_t stream) {
  if (!w_hhT) return ASR_E_ARG;
  return lstm_seq_bwd_persist_impl(T, B, nb, H, ndir, gates, w_hhT, nullptr, lens, rowbase, rowext, lens_host, dy, c, y,
                                   dw_hh, db, xch, ctrl, arith, stream);
}

// Same, taking W_hh in the FORWARD layout ([ndir][4H][H], what asr_lstm_seq_fwd_persist consumed): the exchanged-partials
// kernel reads its slice of it once per launch, so the caller needs no transposed copy.  ASR_E_SHAPE when that kernel
// does not apply (H not in {128, 256, 512}, fp32-MFMA arithmetic, ASR_LSTM_BWD_GATHER): the caller then transposes and uses
// asr_lstm_seq_bwd_persist.
extern "C" int asr_lstm_seq_bwd_persist_w(int T, int B, int nb, int H, int ndir, float* gates, const float* w_hh_il,
                                          const int32_t* lens, const int32_t* rowbase, const int32_t* rowext,
                                          const int32_t* lens_host, const float* dy, const float* c, const float* y,
                                          float* dw_hh, float* db, void* xch, void* ctrl, int arith, asr_stream_t stream) {
  if (!w_hh_il) return ASR_E_ARG;
  return lstm_seq_bwd_persist_impl(T, B, nb, H, ndir, gates, nullptr, w_hh_il, lens, rowbase, rowext, lens_host, dy, c, y,
                                   dw_hh, db, xch, ctrl, arith, stream);
}
