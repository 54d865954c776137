// augment.hip — reverberation and additive noise over packed waveforms, between the resampler and the fbank.
//   reverb_kernel    grid (ceil(longest row / kTile), B), one workgroup of four waves per tile of kTile = 4096 consecutive
//                    output samples of ONE utterance; a wave owns 1024 of them as ONE 32 x 32 fp32 accumulator of
//                    v_mfma_f32_32x32x2_f32.  With n = n0 + 32 a + b:  Y[a][b] = sum_j X[a][j] H[j][b],
//                    X[a][j] = x[n0 + 32 a + 31 + d - j] (a window of the staged input, never materialised),
//                    H[j][b] = h[j - 31 + b] (the RIR as a band, zero outside [0, L)), j = 0 .. L + 30.  The taps are taken in
//                    chunks of kChunk: a chunk [c0, c0 + Lc) is the same product with h + c0 and d - c0, so the workgroup
//                    stages 4096 + Lc input samples (zero-filled outside [0, N), converted from int16 there) and Lc + 64 band
//                    entries per chunk and the accumulator stays in registers across chunks; LDS does not grow with L.
//                    The A operand's lanes are 32 samples apart: the staged span is padded by one word per 32 (index i lives
//                    at i + (i >> 5)), so the 32 lanes of a read fall on 32 banks.  A wave whose 1024 outputs all lie behind
//                    the row's end issues no MFMA.  A row whose RIR index is negative is a copy by value: no LDS, no filter.
//   power_kernel     grid (ceil(longest row / kMixTile), B): the float64 sums of y^2 and v^2 over one tile, each lane over its
//                    elements in ascending order, then a fixed tree over the workgroup -> ws[b][tile][2].
//   mix_kernel       same grid: every workgroup adds the row's partials in tile order, g = scale sqrt(P_y / P_v) in float64
//                    rounded once, z = fmaf(g, v, y); tile 0 writes gains[b].
// Offsets, bank geometry and indices read on the device are clamped into the buffers: wrong values give wrong numbers, never
// an access outside them.  No atomics, no scratch, every sum in a fixed order: the same bits in every run.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = ASR_REVERB_TILE;            // outputs per workgroup: four waves of 32 x 32
constexpr int kWaveTile = 1024;
constexpr int kChunk = ASR_REVERB_CHUNK;          // taps staged at a time
constexpr int kMaxTaps = ASR_REVERB_MAX_TAPS;
constexpr int kSpan = kTile + kChunk;             // staged input samples of one chunk
constexpr int kSpanPadded = kSpan + kSpan / 32;
constexpr int kBand = kChunk + 64;                // 31 zeros | Lc taps | zeros up to the last (padded) step
constexpr int kMixTile = ASR_NOISE_TILE;
static_assert(kTile == 4 * kWaveTile && kThreads == 4 * 64, "one 32 x 32 accumulator per wave");
static_assert(kChunk % 2 == 0 && kMaxTaps % kChunk == 0, "whole chunks, whole k = 2 steps");
static_assert((kSpanPadded + kBand) * 4 <= 40 * 1024, "four workgroups per CU");
static_assert(kMixTile % kThreads == 0, "a lane takes kMixTile / 256 elements");

struct Row {
  int64_t i0, n, q0;                              // first input element, length (clamped to the output's room), first output
};

__device__ inline Row row_of(const int64_t* __restrict__ off, int b, int64_t in_count, int64_t out_count) {
  int64_t i0 = off[b], i1 = off[b + 1];
  i0 = i0 < 0 ? 0 : (i0 > in_count ? in_count : i0);
  i1 = i1 < i0 ? i0 : (i1 > in_count ? in_count : i1);
  int64_t q0 = i0 > out_count ? out_count : i0;   // the output is packed like the input
  int64_t n = i1 - i0;
  n = n > out_count - q0 ? out_count - q0 : n;
  return Row{i0, n, q0};
}

template <typename S>
__global__ __launch_bounds__(kThreads) void reverb_kernel(const S* __restrict__ samples, int64_t in_count,
                                                          const int64_t* __restrict__ off,
                                                          const int32_t* __restrict__ ridx, int n_rirs,
                                                          const int64_t* __restrict__ geo,      // [n_rirs][3]: offset, taps, d
                                                          const float* __restrict__ bank, int64_t bank_count,
                                                          float* __restrict__ out, int64_t out_count) {
  __shared__ float xs[kSpanPadded];
  __shared__ float hs[kBand];
  const int b = blockIdx.y, tid = threadIdx.x;
  const Row r = row_of(off, b, in_count, out_count);
  const int64_t o0 = (int64_t)blockIdx.x * kTile;
  if (o0 >= r.n) return;                           // (the whole workgroup)
  const S* x = samples + r.i0;
  float* y = out + r.q0 + o0;
  const int n_tile = (int)(r.n - o0 < kTile ? r.n - o0 : kTile);
  int ri = ridx[b];
  if (ri < 0) {
    for (int e = tid; e < n_tile; e += kThreads) y[e] = (float)x[o0 + e];
    return;
  }
  ri = ri >= n_rirs ? n_rirs - 1 : ri;
  int64_t h0 = geo[3 * ri], taps = geo[3 * ri + 1], dd = geo[3 * ri + 2];
  h0 = h0 < 0 ? 0 : (h0 > bank_count ? bank_count : h0);
  taps = taps < 0 ? 0 : (taps > kMaxTaps ? kMaxTaps : taps);
  taps = taps > bank_count - h0 ? bank_count - h0 : taps;
  dd = dd < 0 ? 0 : (dd >= taps ? (taps > 0 ? taps - 1 : 0) : dd);
  const int L = (int)taps, d = (int)dd;
  const float* h = bank + h0;

  const int wave = tid >> 6, lane = tid & 63;
  const int a = lane & 31, k = lane >> 5;
  const bool live = wave * kWaveTile < n_tile;     // wave-uniform: this wave has an output inside the row
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int c0 = 0; c0 < L; c0 += kChunk) {
    const int Lc = L - c0 < kChunk ? L - c0 : kChunk;
    if (c0) __syncthreads();                       // the previous chunk's reads are done
    const int64_t first = o0 + (d - c0) - Lc;      // utterance index of staged sample 0; may be negative
    for (int s = tid; s < kTile + Lc; s += kThreads) {
      const int64_t idx = first + s;
      xs[s + (s >> 5)] = idx >= 0 && idx < r.n ? (float)x[idx] : 0.f;
    }
    for (int t = tid; t < Lc + 64; t += kThreads) hs[t] = t >= 31 && t - 31 < Lc ? h[c0 + t - 31] : 0.f;
    __syncthreads();
    if (live) {
      const int steps = (Lc + 32) & ~1;            // j = 0 .. Lc + 30, padded to a whole k = 2 step (a zero row of H)
      const int xi = wave * kWaveTile + 32 * a + 31 + Lc - k;
      const int hi = k + a;
      int j0 = 0;
      for (; j0 + 8 <= steps; j0 += 8) {           // four steps' operands in flight before the first MFMA needs one
        float av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int s = xi - j0 - 2 * u;
          av[u] = xs[s + (s >> 5)];
          bv[u] = hs[hi + j0 + 2 * u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
      }
      for (; j0 < steps; j0 += 2) {
        const int s = xi - j0;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[s + (s >> 5)], hs[hi + j0], acc, 0, 0, 0);
      }
    }
  }
  if (live) {
    // C/D layout: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int e = wave * kWaveTile + 32 * ((i & 3) + 8 * (i >> 2) + 4 * k) + a;
      if (e < n_tile) y[e] = acc[i];
    }
  }
}

// the clip sample behind output element e of a tile whose first element reads clip position m0 (< len)
__device__ inline float clip_at(const float* __restrict__ clip, int64_t len, int64_t m0, int e) {
  int64_t m = m0 + e;
  if (m >= len) {
    m -= len;
    if (m >= len) m %= len;
  }
  return clip[m];
}

struct Clip {
  const float* p;
  int64_t len, start;
};

// -> the row's clip, clamped into the bank; len == 0: no clip
__device__ inline Clip clip_of(const int32_t* __restrict__ cidx, const int64_t* __restrict__ start, int b, int n_clips,
                               const int64_t* __restrict__ coff, const float* __restrict__ bank, int64_t bank_count) {
  int c = cidx[b];
  if (c < 0) return Clip{bank, 0, 0};
  c = c >= n_clips ? n_clips - 1 : c;
  int64_t c0 = coff[c], c1 = coff[c + 1];
  c0 = c0 < 0 ? 0 : (c0 > bank_count ? bank_count : c0);
  c1 = c1 < c0 ? c0 : (c1 > bank_count ? bank_count : c1);
  const int64_t len = c1 - c0;
  int64_t s = start[b];
  s = len > 0 ? (s < 0 ? 0 : s % len) : 0;
  return Clip{bank + c0, len, s};
}

template <typename S>
__global__ __launch_bounds__(kThreads) void power_kernel(const S* __restrict__ samples, int64_t in_count,
                                                         const int64_t* __restrict__ off, const int32_t* __restrict__ cidx,
                                                         const int64_t* __restrict__ start, int n_clips,
                                                         const int64_t* __restrict__ coff, const float* __restrict__ bank,
                                                         int64_t bank_count, int64_t out_count, double* __restrict__ ws) {
  __shared__ double red[2][kThreads];
  const int b = blockIdx.y, tid = threadIdx.x;
  const Row r = row_of(off, b, in_count, out_count);
  const int64_t o0 = (int64_t)blockIdx.x * kMixTile;
  if (o0 >= r.n) return;
  const Clip c = clip_of(cidx, start, b, n_clips, coff, bank, bank_count);
  if (c.len == 0) return;
  const S* x = samples + r.i0 + o0;
  const int n_tile = (int)(r.n - o0 < kMixTile ? r.n - o0 : kMixTile);
  const int64_t m0 = (c.start + o0 % c.len) % c.len;
  double py = 0.0, pv = 0.0;
  for (int e = tid; e < n_tile; e += kThreads) {
    const double yv = (double)(float)x[e], vv = (double)clip_at(c.p, c.len, m0, e);
    py += yv * yv;
    pv += vv * vv;
  }
  red[0][tid] = py;
  red[1][tid] = pv;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (tid < w) {
      red[0][tid] += red[0][tid + w];
      red[1][tid] += red[1][tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* p = ws + 2 * ((int64_t)b * gridDim.x + blockIdx.x);
    p[0] = red[0][0];
    p[1] = red[1][0];
  }
}

template <typename S>
__global__ __launch_bounds__(kThreads) void mix_kernel(const S* samples, int64_t in_count,   // (may be `out`)
                                                       const int64_t* __restrict__ off, const int32_t* __restrict__ cidx,
                                                       const int64_t* __restrict__ start, const float* __restrict__ scale,
                                                       int n_clips, const int64_t* __restrict__ coff,
                                                       const float* __restrict__ bank, int64_t bank_count,
                                                       const double* __restrict__ ws, float* out, int64_t out_count,
                                                       float* __restrict__ gains, int in_place) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const Row r = row_of(off, b, in_count, out_count);
  const int64_t o0 = (int64_t)blockIdx.x * kMixTile;
  const Clip c = clip_of(cidx, start, b, n_clips, coff, bank, bank_count);
  float g = 0.f;
  if (c.len > 0 && r.n > 0) {
    const int tiles = (int)((r.n + kMixTile - 1) / kMixTile);
    const double* p = ws + 2 * (int64_t)b * gridDim.x;
    double py = 0.0, pv = 0.0;
    for (int t = 0; t < tiles; ++t) {              // tile order, the same in every workgroup of the row
      py += p[2 * t];
      pv += p[2 * t + 1];
    }
    if (py > 0.0 && pv > 0.0) g = (float)((double)scale[b] * sqrt(py / pv));
  }
  if (blockIdx.x == 0 && tid == 0 && gains) gains[b] = g;
  if (o0 >= r.n) return;
  const S* x = samples + r.i0 + o0;
  float* z = out + r.q0 + o0;
  const int n_tile = (int)(r.n - o0 < kMixTile ? r.n - o0 : kMixTile);
  if (g == 0.f) {                                  // no clip, or a silent clip / utterance: the row is left as it is
    if (!in_place)
      for (int e = tid; e < n_tile; e += kThreads) z[e] = (float)x[e];
    return;
  }
  const int64_t m0 = (c.start + o0 % c.len) % c.len;
  for (int e = tid; e < n_tile; e += kThreads) z[e] = fmaf(g, clip_at(c.p, c.len, m0, e), (float)x[e]);
}

int common_check(int B, int64_t max_len, const void* samples, int sample_dtype, int64_t in_count, const void* offsets,
                 const void* out, int64_t out_count, int64_t tile, int64_t* tiles) {
  if (!samples || !offsets || !out || B <= 0 || max_len <= 0 || in_count < 0 || out_count < 0) return ASR_E_ARG;
  if (sample_dtype != ASR_SAMPLES_I16 && sample_dtype != ASR_SAMPLES_F32) return ASR_E_SHAPE;
  *tiles = (max_len + tile - 1) / tile;
  if (B > 65535 || *tiles > 0x7fffffff) return ASR_E_SHAPE;
  if ((((uintptr_t)out) & 3u) != 0 || (((uintptr_t)samples) & (sample_dtype == ASR_SAMPLES_I16 ? 1u : 3u)) != 0)
    return ASR_E_ALIGN;
  return 0;
}

}  // namespace

extern "C" int asr_reverb_f32(int B, int64_t max_len, const void* samples, int sample_dtype, int64_t in_count,
                              const int64_t* offsets, const int32_t* rir_index, int n_rirs, const int64_t* geometry,
                              const int64_t* geometry_dev, const float* bank, int64_t bank_count, float* out,
                              int64_t out_count, asr_stream_t stream) {
  int64_t tiles = 0;
  const int rc = common_check(B, max_len, samples, sample_dtype, in_count, offsets, out, out_count, kTile, &tiles);
  if (rc) return rc;
  if (!rir_index || !geometry || !geometry_dev || !bank || n_rirs <= 0 || bank_count <= 0) return ASR_E_ARG;
  if ((const void*)samples == (const void*)out) return ASR_E_ARG;           // a tile reads its neighbours' input
  for (int i = 0; i < n_rirs; ++i) {
    const int64_t h0 = geometry[3 * i], taps = geometry[3 * i + 1], d = geometry[3 * i + 2];
    if (taps > kMaxTaps) return ASR_E_SHAPE;
    if (h0 < 0 || taps <= 0 || h0 + taps > bank_count || d < 0 || d >= taps) return ASR_E_ARG;
  }
  if ((((uintptr_t)bank) & 3u) != 0 || (((uintptr_t)geometry_dev) & 7u) != 0) return ASR_E_ALIGN;
  const dim3 grid((unsigned)tiles, (unsigned)B);
  if (sample_dtype == ASR_SAMPLES_I16)
    hipLaunchKernelGGL((reverb_kernel<int16_t>), grid, dim3(kThreads), 0, (hipStream_t)stream, (const int16_t*)samples,
                       in_count, offsets, rir_index, n_rirs, geometry_dev, bank, bank_count, out, out_count);
  else
    hipLaunchKernelGGL((reverb_kernel<float>), grid, dim3(kThreads), 0, (hipStream_t)stream, (const float*)samples, in_count,
                       offsets, rir_index, n_rirs, geometry_dev, bank, bank_count, out, out_count);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_noise_mix_f32(int B, int64_t max_len, const void* samples, int sample_dtype, int64_t in_count,
                                 const int64_t* offsets, const int32_t* clip_index, const int64_t* start, const float* scale,
                                 int n_clips, const int64_t* clip_offsets, const int64_t* clip_offsets_dev, const float* bank,
                                 int64_t bank_count, void* ws, int64_t ws_bytes, float* out, int64_t out_count, float* gains,
                                 asr_stream_t stream) {
  int64_t tiles = 0;
  const int rc = common_check(B, max_len, samples, sample_dtype, in_count, offsets, out, out_count, kMixTile, &tiles);
  if (rc) return rc;
  if (!clip_index || !start || !scale || !clip_offsets || !clip_offsets_dev || !bank || !ws || n_clips <= 0 || bank_count <= 0)
    return ASR_E_ARG;
  if (clip_offsets[0] < 0 || clip_offsets[n_clips] > bank_count) return ASR_E_ARG;
  for (int i = 0; i < n_clips; ++i)
    if (clip_offsets[i + 1] <= clip_offsets[i]) return ASR_E_ARG;
  if (ws_bytes < 16 * (int64_t)B * tiles) return ASR_E_ARG;
  const int in_place = (const void*)samples == (const void*)out;
  if (in_place && sample_dtype != ASR_SAMPLES_F32) return ASR_E_ARG;
  if ((((uintptr_t)bank) & 3u) != 0 || (((uintptr_t)ws) & 7u) != 0 || (((uintptr_t)clip_offsets_dev) & 7u) != 0 ||
      (((uintptr_t)scale) & 3u) != 0 || (gains && (((uintptr_t)gains) & 3u) != 0))
    return ASR_E_ALIGN;
  const dim3 grid((unsigned)tiles, (unsigned)B);
  if (sample_dtype == ASR_SAMPLES_I16) {
    hipLaunchKernelGGL((power_kernel<int16_t>), grid, dim3(kThreads), 0, (hipStream_t)stream, (const int16_t*)samples,
                       in_count, offsets, clip_index, start, n_clips, clip_offsets_dev, bank, bank_count, out_count,
                       (double*)ws);
    ASR_CHECK_LAUNCH();
    hipLaunchKernelGGL((mix_kernel<int16_t>), grid, dim3(kThreads), 0, (hipStream_t)stream, (const int16_t*)samples, in_count,
                       offsets, clip_index, start, scale, n_clips, clip_offsets_dev, bank, bank_count, (const double*)ws, out,
                       out_count, gains, in_place);
  } else {
    hipLaunchKernelGGL((power_kernel<float>), grid, dim3(kThreads), 0, (hipStream_t)stream, (const float*)samples, in_count,
                       offsets, clip_index, start, n_clips, clip_offsets_dev, bank, bank_count, out_count, (double*)ws);
    ASR_CHECK_LAUNCH();
    hipLaunchKernelGGL((mix_kernel<float>), grid, dim3(kThreads), 0, (hipStream_t)stream, (const float*)samples, in_count,
                       offsets, clip_index, start, scale, n_clips, clip_offsets_dev, bank, bank_count, (const double*)ws, out,
                       out_count, gains, in_place);
  }
  ASR_CHECK_LAUNCH();
  return 0;
}
