// resample.hip — speed perturbation: a polyphase resampler over packed waveforms.
//   resample_kernel  grid (ceil(longest output / kTile), B), one workgroup of four waves per tile of kTile consecutive output
//                    samples of ONE utterance.  Utterance b carries factor f = factor_index[b]: orig / new in lowest terms, a
//                    bank h[new][taps] of Hann-windowed sinc taps from the caller's table buffer (float64 on the host, rounded
//                    to fp32: no sine, cosine or division per tap here).  Output o = i new + j is sum_k h[j][k] x[i orig + k -
//                    width], x zero outside the utterance.  The workgroup stages the tile's input span ((i_last - i_first)
//                    orig + taps samples, zero-filled outside [0, n), converted from int16 there) and the factor's bank in LDS
//                    once; a lane then forms four outputs, each one running fp32 sum (fmaf) over k = 0 .. taps - 1.
//                    A factor with orig == new == 1 is a copy by value: no filter, no LDS.
// The output length of a row is ceil(new n / orig), computed here and clamped to the room out_offsets leaves; offsets are
// clamped into [0, in_count] / [0, out_count]: wrong offsets give wrong numbers, never an access outside the two buffers.
// No atomics, no scratch, every sum in a fixed order: the same bits in every run.
#include "common.h"

namespace {

constexpr int kTile = ASR_RESAMPLE_TILE;
constexpr int kMaxF = ASR_RESAMPLE_MAX_FACTORS;
constexpr int kMaxPhases = ASR_RESAMPLE_MAX_PHASES;
constexpr int kMaxTaps = ASR_RESAMPLE_MAX_TAPS;
constexpr int kMaxSpan = ASR_RESAMPLE_MAX_SPAN;
constexpr int kThreads = 256;
static_assert(kTile % kThreads == 0, "a lane forms kTile / 256 outputs");

struct Geom {                       // by value in the kernel's arguments; entries behind n are zero
  int n;
  int orig[kMaxF], nw[kMaxF], width[kMaxF], taps[kMaxF], off[kMaxF];
};

// the input span a tile may need: its blocks i_first .. i_last cover at most (kTile - 1) / new + 2 block starts
inline int64_t max_span(int orig, int nw, int taps) { return ((int64_t)(kTile - 1) / nw + 1) * orig + taps; }

// -> 0, or ASR_E_SHAPE / ASR_E_ARG; *floats = the table floats the geometry addresses
int geom_check(int n_factors, const int32_t* g, int64_t* floats) {
  if (!g || n_factors <= 0) return ASR_E_ARG;
  if (n_factors > kMaxF) return ASR_E_SHAPE;
  int64_t end = 0;
  for (int f = 0; f < n_factors; ++f) {
    const int orig = g[5 * f], nw = g[5 * f + 1], width = g[5 * f + 2], taps = g[5 * f + 3], off = g[5 * f + 4];
    if (orig <= 0 || nw <= 0 || width < 0 || taps <= 0 || off < 0) return ASR_E_ARG;
    if (nw > kMaxPhases || taps > kMaxTaps) return ASR_E_SHAPE;
    if (taps != 2 * width + orig) return ASR_E_ARG;
    if (max_span(orig, nw, taps) > kMaxSpan) return ASR_E_SHAPE;
    const int64_t e = (int64_t)off + (int64_t)nw * taps;
    end = e > end ? e : end;
  }
  *floats = end;
  return 0;
}

template <typename S>
__global__ __launch_bounds__(kThreads) void resample_kernel(Geom g, const S* __restrict__ samples, int64_t in_count,
                                                            const int64_t* __restrict__ in_off,
                                                            const int32_t* __restrict__ fidx,
                                                            const int64_t* __restrict__ out_off,
                                                            const float* __restrict__ tables, float* __restrict__ out,
                                                            int64_t out_count) {
  __shared__ float xs[kMaxSpan];
  __shared__ float hs[kMaxPhases * kMaxTaps];
  const int b = blockIdx.y, tid = threadIdx.x;
  int f = fidx[b];
  f = f < 0 ? 0 : (f >= g.n ? g.n - 1 : f);
  int orig = 1, nw = 1, width = 0, taps = 1, off = 0;
#pragma unroll
  for (int i = 0; i < kMaxF; ++i)                  // constant indices: the argument block is never indexed by a register
    if (i == f) { orig = g.orig[i]; nw = g.nw[i]; width = g.width[i]; taps = g.taps[i]; off = g.off[i]; }
  int64_t i0 = in_off[b], i1 = in_off[b + 1];
  i0 = i0 < 0 ? 0 : (i0 > in_count ? in_count : i0);
  i1 = i1 < i0 ? i0 : (i1 > in_count ? in_count : i1);
  const int64_t n = i1 - i0;
  int64_t q0 = out_off[b], q1 = out_off[b + 1];
  q0 = q0 < 0 ? 0 : (q0 > out_count ? out_count : q0);
  q1 = q1 < q0 ? q0 : (q1 > out_count ? out_count : q1);
  int64_t n_out = (n * nw + orig - 1) / orig;      // once per workgroup
  n_out = n_out > q1 - q0 ? q1 - q0 : n_out;
  const int64_t o0 = (int64_t)blockIdx.x * kTile;
  if (o0 >= n_out) return;                         // (the whole workgroup)
  const S* x = samples + i0;
  float* y = out + q0 + o0;
  const int n_tile = (int)(n_out - o0 < kTile ? n_out - o0 : kTile);
  if (orig == 1 && nw == 1) {
    for (int e = tid; e < n_tile; e += kThreads) y[e] = (float)x[o0 + e];
    return;
  }
  const int64_t blk0 = o0 / nw;                    // the tile's first input block
  const int ph0 = (int)(o0 - blk0 * nw);           // and the phase of its first output
  const int blk_span = (ph0 + n_tile - 1) / nw;    // i_last - i_first
  int span = blk_span * orig + taps;
  span = span > kMaxSpan ? kMaxSpan : span;        // (the host refuses such geometry: never taken)
  const int64_t first = blk0 * orig - width;       // utterance index of xs[0]; negative at the head
  for (int s = tid; s < span; s += kThreads) {
    const int64_t idx = first + s;
    xs[s] = idx >= 0 && idx < n ? (float)x[idx] : 0.f;
  }
  for (int e = tid; e < nw * taps; e += kThreads) hs[e] = tables[off + e];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kTile / kThreads; ++r) {
    const int e = r * kThreads + tid;
    if (e < n_tile) {
      const int rel = (ph0 + e) / nw, j = (ph0 + e) - rel * nw;
      const float* xp = xs + rel * orig;
      const float* hp = hs + j * taps;
      float acc = 0.f;
      for (int k = 0; k < taps; ++k) acc = fmaf(hp[k], xp[k], acc);
      y[e] = acc;
    }
  }
}

}  // namespace

extern "C" int asr_resample_plan_bytes(int n_factors, const int32_t* geometry, int64_t* bytes) {
  if (!bytes) return ASR_E_ARG;
  int64_t floats = 0;
  const int rc = geom_check(n_factors, geometry, &floats);
  if (rc) return rc;
  *bytes = 4 * floats;
  return 0;
}

extern "C" int asr_resample_f32(int B, int64_t max_out, const void* samples, int sample_dtype, int64_t in_count,
                                const int64_t* in_offsets, const int32_t* factor_index, const int64_t* out_offsets,
                                int n_factors, const int32_t* geometry, const void* tables, int64_t table_bytes, float* out,
                                int64_t out_count, asr_stream_t stream) {
  if (!samples || !in_offsets || !factor_index || !out_offsets || !tables || !out || B <= 0 || max_out <= 0 || in_count < 0 ||
      out_count < 0)
    return ASR_E_ARG;
  if (sample_dtype != ASR_SAMPLES_I16 && sample_dtype != ASR_SAMPLES_F32) return ASR_E_SHAPE;
  int64_t floats = 0;
  const int rc = geom_check(n_factors, geometry, &floats);
  if (rc) return rc;
  if (4 * floats > table_bytes) return ASR_E_ARG;
  const int64_t tiles = (max_out + kTile - 1) / kTile;
  if (B > 65535 || tiles > 0x7fffffff) return ASR_E_SHAPE;
  if ((((uintptr_t)tables) & 3u) != 0 || (((uintptr_t)out) & 3u) != 0 ||
      (((uintptr_t)samples) & (sample_dtype == ASR_SAMPLES_I16 ? 1u : 3u)) != 0)
    return ASR_E_ALIGN;
  Geom g = {};
  g.n = n_factors;
  for (int f = 0; f < n_factors; ++f) {
    g.orig[f] = geometry[5 * f];
    g.nw[f] = geometry[5 * f + 1];
    g.width[f] = geometry[5 * f + 2];
    g.taps[f] = geometry[5 * f + 3];
    g.off[f] = geometry[5 * f + 4];
  }
  const dim3 grid((unsigned)tiles, (unsigned)B);
  if (sample_dtype == ASR_SAMPLES_I16)
    hipLaunchKernelGGL((resample_kernel<int16_t>), grid, dim3(kThreads), 0, (hipStream_t)stream, g, (const int16_t*)samples,
                       in_count, in_offsets, factor_index, out_offsets, (const float*)tables, out, out_count);
  else
    hipLaunchKernelGGL((resample_kernel<float>), grid, dim3(kThreads), 0, (hipStream_t)stream, g, (const float*)samples,
                       in_count, in_offsets, factor_index, out_offsets, (const float*)tables, out, out_count);
  ASR_CHECK_LAUNCH();
  return 0;
}
