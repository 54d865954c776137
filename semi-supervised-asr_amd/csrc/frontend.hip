// frontend.hip — from packed waveforms to the [B][T][D] tensor the encoder reads.
//   fbank_kernel       Kaldi-convention (log-)mel filterbank energies, dither off, snip-edges.  One workgroup of four waves
//                      per tile of kFrameTile = 8 consecutive frames of one utterance, one wave per frame, two frames per
//                      wave.  A wave reads its frame's L samples (element by element: an int16 utterance may start at an odd
//                      element, and nothing outside [offsets[b], offsets[b+1]) is touched), subtracts the frame mean,
//                      pre-emphasises, windows and zero-pads into LDS, where the n_fft real points ARE the n_fft / 2 complex
//                      points z[n] = x[2n] + i x[2n+1].  A radix-2 decimation-in-frequency FFT of z runs in place (results in
//                      bit-reversed order), the untangle pass turns Z into bins 0 .. n_fft/2 - 1 of the real spectrum and
//                      writes their power, and every lane sums its mel bins over a [start, len] range of packed weights in
//                      ascending bin order (a compensated sum).  Window, twiddles and mel weights come from the caller's plan
//                      buffer (float64 on the host, rounded to fp32): no sine or cosine is evaluated here.
//   cmvn_stats_kernel  per utterance and bin: mean and 1 / sqrt(max(biased variance, 1e-10)) over the utterance's frames, two
//                      passes (the variance about the mean), four row groups per bin combined in a fixed order.
//   finish_kernel      CMVN of the static features, deltas (Kaldi add-deltas, window 2, each order a filter over the STATIC
//                      rows with the frame index clamped), SpecAugment masks, exact zeros behind an utterance.
// No floating-point atomics, every sum in an order fixed by the shapes: the same bits in every run.
#include <float.h>
#include <math.h>
#include "common.h"

namespace {

constexpr int kFrameTile = ASR_FBANK_FRAME_TILE;
constexpr int kMaxMels = ASR_FBANK_MAX_MELS;
static_assert(kFrameTile % 4 == 0, "a tile is shared by four waves");

// the plan: 4-byte words, see include/asr_hip.h
struct PlanView {
  const float* window;    // [n_fft]      zero behind the frame length
  const float* tw;        // [n_fft / 2]  (cos, -sin)(2 pi j / M), j < M / 2, M = n_fft / 2
  const float* ut;        // [n_fft]      (cos, -sin)(2 pi k / n_fft), k < M
  const int32_t* start;   // [kMaxMels]
  const int32_t* len;     // [kMaxMels]
  const int32_t* woff;    // [kMaxMels]
  const float* w;         // [n_fft]
};

inline int64_t plan_words(int n_fft) { return (int64_t)n_fft * 7 / 2 + 3 * kMaxMels; }

__host__ __device__ inline PlanView plan_view(const void* plan, int n_fft) {
  PlanView p;
  p.window = (const float*)plan;
  p.tw = p.window + n_fft;
  p.ut = p.tw + n_fft / 2;
  p.start = (const int32_t*)(p.ut + n_fft);
  p.len = p.start + kMaxMels;
  p.woff = p.len + kMaxMels;
  p.w = (const float*)(p.woff + kMaxMels);
  return p;
}

__host__ __device__ inline int64_t num_frames(int64_t n, int L, int S) { return n >= L ? 1 + (n - L) / S : 0; }

template <typename S>
__device__ __forceinline__ float sample_f32(const S* p, int64_t i) { return (float)p[i]; }

template <typename S, int NFFT>
__global__ __launch_bounds__(256) void fbank_kernel(int T_max, const S* __restrict__ samples,
                                                    const int64_t* __restrict__ offsets, int L, int shift, int n_mels,
                                                    float preemph, int use_log, float log_floor, const void* plan,
                                                    float* __restrict__ out, int64_t ld, int64_t col0) {
  constexpr int M = NFFT / 2;                      // complex points
  constexpr int LOGM = NFFT == 512 ? 8 : 7;
  __shared__ float zs[4][NFFT];                    // per wave: the frame, then z / Z interleaved (re, im)
  __shared__ float pw[4][M];                       // per wave: the power spectrum, bins 0 .. M - 1
  const int b = blockIdx.y, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int64_t o0 = offsets[b];
  int64_t Tb = num_frames(offsets[b + 1] - o0, L, shift);
  Tb = Tb > T_max ? T_max : Tb;
  const int64_t t0 = (int64_t)blockIdx.x * kFrameTile;
  if (t0 >= Tb) return;                            // (the whole workgroup)
  const PlanView p = plan_view(plan, NFFT);
  float* z = zs[wave];
  float* pz = pw[wave];
  for (int r = 0; r < kFrameTile / 4; ++r) {
    const int64_t t = t0 + r * 4 + wave;
    const bool act = t < Tb;                       // wave-uniform; the barriers below are reached by every wave
    if (act) {
      const S* x = samples + o0 + t * shift;       // samples [0, L) of the frame lie inside the utterance
      float s = 0.f;
      for (int n = lane; n < L; n += 64) s += sample_f32(x, n);
      const float mean = wave_sum(s) / (float)L;
      for (int n = lane; n < NFFT; n += 64) {
        float v = 0.f;
        if (n < L) {
          const float a = sample_f32(x, n) - mean;
          const float c = sample_f32(x, n > 0 ? n - 1 : 0) - mean;
          v = (a - preemph * c) * p.window[n];
        }
        z[n] = v;
      }
    }
    __syncthreads();
    // decimation in frequency: half = M/2, M/4, ..., 1; butterfly j pairs i0 = (j / half) 2 half + j % half with i0 + half
    // and turns the difference by W_M^{(j % half) (M / (2 half))}
#pragma unroll
    for (int s = 0; s < LOGM; ++s) {
      const int half = M >> (s + 1);
      if (act) {
#pragma unroll
        for (int j0 = 0; j0 < M / 2; j0 += 64) {
          const int j = j0 + lane;
          const int pos = j & (half - 1);
          const int i0 = ((j >> (LOGM - 1 - s)) << (LOGM - s)) + pos, i1 = i0 + half;
          const int k = pos << s;
          const float wr = p.tw[2 * k], wi = p.tw[2 * k + 1];
          const float ar = z[2 * i0], ai = z[2 * i0 + 1], br = z[2 * i1], bi = z[2 * i1 + 1];
          const float dr = ar - br, di = ai - bi;
          z[2 * i0] = ar + br;
          z[2 * i0 + 1] = ai + bi;
          z[2 * i1] = dr * wr - di * wi;
          z[2 * i1 + 1] = dr * wi + di * wr;
        }
      }
      __syncthreads();
    }
    // untangle: with Zk = Z[k], Zm = conj(Z[(M - k) mod M]):  X[k] = (Zk + Zm)/2 - i w_k (Zk - Zm)/2, w_k = e^{-2 pi i k / n_fft}
    if (act) {
#pragma unroll
      for (int k0 = 0; k0 < M; k0 += 64) {
        const int k = k0 + lane;
        const int ik = (int)(__brev((unsigned)k) >> (32 - LOGM));
        const int im = (int)(__brev((unsigned)((M - k) & (M - 1))) >> (32 - LOGM));
        const float kr = z[2 * ik], ki = z[2 * ik + 1], mr = z[2 * im], mi = -z[2 * im + 1];
        const float er = 0.5f * (kr + mr), ei = 0.5f * (ki + mi), dr = 0.5f * (kr - mr), di = 0.5f * (ki - mi);
        const float wr = p.ut[2 * k], wi = p.ut[2 * k + 1];
        // -i w d = (wr di + wi dr) + i (wi di - wr dr)
        const float xr = er + (wr * di + wi * dr), xi = ei + (wi * di - wr * dr);
        pz[k] = xr * xr + xi * xi;
      }
    }
    __syncthreads();
    if (act) {
      float* row = out + ((int64_t)b * T_max + t) * ld + col0;
      for (int j = lane; j < n_mels; j += 64) {
        int st = p.start[j], ln = p.len[j], wo = p.woff[j];
        st = st < 0 ? 0 : (st > M ? M : st);               // a plan that is wrong reads wrong weights, never out of bounds
        ln = ln < 0 ? 0 : (ln > M - st ? M - st : ln);
        wo = wo < 0 ? 0 : (wo > NFFT - ln ? NFFT - ln : wo);
        // compensated (Kahan) sum in ascending bin order: a filter may span all n_fft / 2 bins (n_mels = 1), and a plain
        // fp32 running sum of that many terms alone would cost several 2^-24 of the frame's largest energy
        float e = 0.f, comp = 0.f;
        for (int i = 0; i < ln; ++i) {
          const float y = p.w[wo + i] * pz[st + i] - comp;
          const float u = e + y;
          comp = (u - e) - y;
          e = u;
        }
        row[j] = use_log ? (e > FLT_EPSILON ? logf(e) : log_floor) : e;
      }
    }
    __syncthreads();                               // pz and z are free for the wave's next frame
  }
}

__global__ __launch_bounds__(512) void cmvn_stats_kernel(int T, int n_mels, const float* __restrict__ x, int64_t ld,
                                                         const int32_t* __restrict__ lens, float* __restrict__ stats) {
  __shared__ float part[4][kMaxMels];
  __shared__ float mean_s[kMaxMels];
  const int b = blockIdx.x, j = threadIdx.x & (kMaxMels - 1), g = threadIdx.x >> 7;
  int len = lens[b];
  len = len < 0 ? 0 : (len > T ? T : len);
  const float* xb = x + (int64_t)b * T * ld;
  const float inv = 1.f / (float)(len > 0 ? len : 1);
  float s = 0.f;
  if (j < n_mels)
    for (int t = g; t < len; t += 4) s += xb[(int64_t)t * ld + j];
  part[g][j] = s;
  __syncthreads();
  if (g == 0) mean_s[j] = ((part[0][j] + part[1][j]) + (part[2][j] + part[3][j])) * inv;
  __syncthreads();
  const float mean = mean_s[j];
  float q = 0.f;
  if (j < n_mels)
    for (int t = g; t < len; t += 4) {
      const float d = xb[(int64_t)t * ld + j] - mean;
      q += d * d;
    }
  part[g][j] = q;
  __syncthreads();
  if (g == 0 && j < n_mels) {
    const float var = ((part[0][j] + part[1][j]) + (part[2][j] + part[3][j])) * inv;
    float* sb = stats + (int64_t)b * 2 * n_mels;
    sb[j] = mean;
    sb[n_mels + j] = 1.f / sqrtf(fmaxf(var, 1e-10f));
  }
}

// Kaldi add-deltas, window 2: s1 = (-2 .. 2) / 10, s2 = s1 * s1
__constant__ float kDelta1[5] = {-0.2f, -0.1f, 0.f, 0.1f, 0.2f};
__constant__ float kDelta2[9] = {0.04f, 0.04f, 0.01f, -0.04f, -0.1f, -0.04f, 0.01f, 0.04f, 0.04f};

__global__ __launch_bounds__(256) void finish_kernel(int T, int n_mels, int order, const float* __restrict__ x, int64_t ldx,
                                                     const int32_t* __restrict__ lens, int cmvn, const float* __restrict__ stats,
                                                     const int32_t* __restrict__ masks, int n_fm, int n_tm,
                                                     float* __restrict__ out) {
  const int b = blockIdx.y;
  const int D = n_mels * (1 + order);
  int len = lens[b];
  len = len < 0 ? 0 : (len > T ? T : len);
  const float* xb = x + (int64_t)b * T * ldx;
  float* ob = out + (int64_t)b * T * D;
  const float* st = cmvn == ASR_CMVN_UTTERANCE ? stats + (int64_t)b * 2 * n_mels : stats;
  const int32_t* mb = masks ? masks + (int64_t)b * (n_fm + n_tm) * 2 : nullptr;
  const int64_t n = (int64_t)T * D;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int t = (int)(e / D), c = (int)(e % D);
    const int k = c / n_mels, j = c % n_mels;
    bool zero = t >= len;
    if (mb && !zero) {
      for (int m = 0; m < n_fm; ++m) {
        const int f0 = mb[2 * m], w = mb[2 * m + 1];
        zero = zero || (w > 0 && j >= f0 && j - f0 < w);
      }
      for (int m = n_fm; m < n_fm + n_tm; ++m) {
        const int s0 = mb[2 * m], w = mb[2 * m + 1];
        zero = zero || (w > 0 && t >= s0 && t - s0 < w);
      }
    }
    float v = 0.f;
    if (!zero) {
      const float mean = cmvn ? st[j] : 0.f, istd = cmvn ? st[n_mels + j] : 1.f;
      if (k == 0) {
        v = xb[(int64_t)t * ldx + j];
        if (cmvn) v = (v - mean) * istd;
      } else {
        const int W = 2 * k;                                  // taps -W .. W
        const float* taps = k == 1 ? kDelta1 : kDelta2;
        for (int d = -W; d <= W; ++d) {
          int u = t + d;
          u = u < 0 ? 0 : (u > len - 1 ? len - 1 : u);
          float a = xb[(int64_t)u * ldx + j];
          if (cmvn) a = (a - mean) * istd;
          v += taps[d + W] * a;
        }
      }
    }
    ob[e] = v;
  }
}

int fbank_check(int L, int S, int n_fft, int n_mels) {
  if (L <= 0 || S <= 0 || n_fft <= 0 || n_mels <= 0) return ASR_E_ARG;
  if ((n_fft != 256 && n_fft != 512) || L > n_fft || n_mels > kMaxMels) return ASR_E_SHAPE;
  return 0;
}

template <typename S>
void fbank_launch(int B, int T_max, const void* samples, const int64_t* offsets, int L, int shift, int n_fft, int n_mels,
                  float preemph, int use_log, const void* plan, float* out, int64_t ld, int64_t col0, hipStream_t stream) {
  const dim3 grid((unsigned)((T_max + kFrameTile - 1) / kFrameTile), (unsigned)B);
  const float log_floor = (float)log((double)FLT_EPSILON);
  if (n_fft == 512)
    hipLaunchKernelGGL((fbank_kernel<S, 512>), grid, dim3(256), 0, stream, T_max, (const S*)samples, offsets, L, shift, n_mels,
                       preemph, use_log, log_floor, plan, out, ld, col0);
  else
    hipLaunchKernelGGL((fbank_kernel<S, 256>), grid, dim3(256), 0, stream, T_max, (const S*)samples, offsets, L, shift, n_mels,
                       preemph, use_log, log_floor, plan, out, ld, col0);
}

}  // namespace

extern "C" int asr_fbank_num_frames(int64_t n_samples, int frame_length, int frame_shift, int64_t* n_frames) {
  if (!n_frames || frame_length <= 0 || frame_shift <= 0 || n_samples < 0) return ASR_E_ARG;
  *n_frames = num_frames(n_samples, frame_length, frame_shift);
  return 0;
}

extern "C" int asr_fbank_plan_bytes(int n_fft, int64_t* bytes) {
  if (!bytes) return ASR_E_ARG;
  if (n_fft != 256 && n_fft != 512) return ASR_E_SHAPE;
  *bytes = 4 * plan_words(n_fft);
  return 0;
}

extern "C" int asr_fbank_f32(int B, int T_max, const void* samples, int sample_dtype, const int64_t* offsets,
                             int frame_length, int frame_shift, int n_fft, int n_mels, float preemph, int use_log,
                             const void* plan, float* out, int64_t ld, int64_t col0, asr_stream_t stream) {
  if (!samples || !offsets || !plan || !out || B <= 0 || T_max <= 0 || col0 < 0 || ld < col0 + n_mels) return ASR_E_ARG;
  if (sample_dtype != ASR_SAMPLES_I16 && sample_dtype != ASR_SAMPLES_F32) return ASR_E_ARG;
  const int rc = fbank_check(frame_length, frame_shift, n_fft, n_mels);
  if (rc) return rc;
  if (B > 65535) return ASR_E_SHAPE;
  if ((((uintptr_t)plan) & 3u) != 0 || (((uintptr_t)samples) & (sample_dtype == ASR_SAMPLES_I16 ? 1u : 3u)) != 0)
    return ASR_E_ALIGN;
  if (sample_dtype == ASR_SAMPLES_I16)
    fbank_launch<int16_t>(B, T_max, samples, offsets, frame_length, frame_shift, n_fft, n_mels, preemph, use_log, plan, out, ld,
                          col0, (hipStream_t)stream);
  else
    fbank_launch<float>(B, T_max, samples, offsets, frame_length, frame_shift, n_fft, n_mels, preemph, use_log, plan, out, ld,
                        col0, (hipStream_t)stream);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_feat_cmvn_stats_f32(int B, int T, int n_mels, const float* x, int64_t ld, const int32_t* frame_lens,
                                       float* stats, asr_stream_t stream) {
  if (!x || !frame_lens || !stats || B <= 0 || T <= 0 || n_mels <= 0 || ld < n_mels) return ASR_E_ARG;
  if (n_mels > kMaxMels) return ASR_E_SHAPE;
  hipLaunchKernelGGL(cmvn_stats_kernel, dim3(B), dim3(512), 0, (hipStream_t)stream, T, n_mels, x, ld, frame_lens, stats);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_feat_finish_f32(int B, int T, int n_mels, int order, const float* x, int64_t ldx, const int32_t* frame_lens,
                                   int cmvn_mode, const float* stats, const int32_t* masks, int n_freq_masks, int n_time_masks,
                                   float* out, asr_stream_t stream) {
  if (!x || !frame_lens || !out || B <= 0 || T <= 0 || n_mels <= 0 || ldx < n_mels) return ASR_E_ARG;
  if (cmvn_mode != ASR_CMVN_NONE && cmvn_mode != ASR_CMVN_GLOBAL && cmvn_mode != ASR_CMVN_UTTERANCE) return ASR_E_ARG;
  if (cmvn_mode != ASR_CMVN_NONE && !stats) return ASR_E_ARG;
  if (n_freq_masks < 0 || n_time_masks < 0 || (n_freq_masks + n_time_masks > 0 && !masks)) return ASR_E_ARG;
  if (order < 0 || order > 2 || n_mels > kMaxMels || B > 65535) return ASR_E_SHAPE;
  const int64_t n = (int64_t)T * n_mels * (1 + order);
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(finish_kernel, dim3((unsigned)(blocks > 1024 ? 1024 : blocks), (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, T, n_mels, order, x, ldx, frame_lens, cmvn_mode, stats,
                     n_freq_masks + n_time_masks > 0 ? masks : nullptr, n_freq_masks, n_time_masks, out);
  ASR_CHECK_LAUNCH();
  return 0;
}
