// ctc_beam.hip — CTC prefix beam search over the CTC head's logits: the n-best list of the head itself, the
// first pass of two-pass decoding.  The conventions are seq_common.h's; its frame_lse_kernel runs first.
//   ctc_beam_kernel       one workgroup per utterance (one wave when K V <= kOneWaveKV, four beyond), looping over its frames.
//                         The beam (at most K prefixes: pb, pnb, tot, last token, length, 64-bit prefix hash) lives in LDS, two
//                         slots.  Per frame:
//                           merge map  thread j < live: the beam entries that are prefix_j + one token (hash of the extension,
//                                      length + 1) as a bit mask - those extensions are not candidates
//                           candidates thread j < live forms the stay candidate of entry j (flat index j), the masses of the
//                                      extensions that ARE entry j added to its pnb' in ascending entry order; all threads walk
//                                      the extensions (entry-major, tokens strided over the threads: ascending flat index
//                                      K + k (V - 1) + (c - 1)) and keep their best M >= K in a sorted register list (top_insert)
//                           select     K rounds of a workgroup arg-best over the list heads (seq_common.h's order; -inf
//                                      never wins); the thread whose number is the round keeps the winner
//                           update     thread r < selected writes entry r of the other slot and (parent slot, token) of the
//                                      frame into the history - LDS when T_b K entries fit kHistLds, the workspace otherwise
//                         The emissions of the frame ahead are in registers (kStage tokens per thread) while a frame runs and go
//                         to LDS at its end; a token behind kStage * threads is read from memory where it is used.
//                         After the last frame the beam IS the ranking (the select's order); thread r walks the history back
//                         into hyp[r].
#include "seq_common.h"

namespace {

constexpr int kKmax = ASR_BEAM_KMAX;
constexpr int kStage = 4;                                  // emissions a thread holds a frame ahead
constexpr int kMaxThreads = 256;
constexpr int kOneWaveKV = ASR_CTC_BEAM_ONE_WAVE_KV;       // K V up to this: one wave per utterance
constexpr int kHistLds = ASR_CTC_BEAM_LDS_ENTRIES;         // (frame, slot) history entries that stay in LDS
static_assert(kKmax <= 32, "the merge map of an entry is one 32-bit mask");
static_assert(kHistLds * 8 + kStage * kMaxThreads * 4 + 2048 <= 64 * 1024, "the static LDS of a workgroup");

typedef unsigned long long u64;

struct BeamWs {
  int2* hist;      // [B][T][K] (parent slot, token; token 0: the entry stayed); absent when T K entries fit LDS
  float* lse;      // [B][T]
  int64_t bytes;
};

BeamWs beam_ws(void* base, int B, int T, int K) {
  const int64_t n_h = (int64_t)T * K > kHistLds ? (int64_t)B * T * K : 0;
  BeamWs w;
  w.hist = (int2*)base;                                      // (first: 8-byte aligned wherever the workspace is)
  w.lse = (float*)(w.hist + n_h);
  w.bytes = 8 * n_h + 4 * round64((int64_t)B * T);
  return w;
}

// log(exp a + exp b); (-inf) (+) (-inf) = -inf, and -inf (+) x = x exactly
// (not ctc_prefix.hip's lae: log1pf here, logf(1 + .) there - they round differently, and each search's bits are its own)
__device__ __forceinline__ float logaddexp(float a, float b) {
  const float m = fmaxf(a, b), n = fminf(a, b);
  if (n == -INFINITY) return m;
  return m + log1pf(expf(n - m));
}

// the hash of prefix . c from the hash of prefix (the splitmix64 finaliser over hash + token): with the length and the last
// token it stands for the token sequence
__device__ __forceinline__ u64 prefix_hash(u64 h, int c) {
  h += (u64)(unsigned)c + 0x9E3779B97F4A7C15ull;
  h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
  h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
  return h ^ (h >> 31);
}

template <int M>
__global__ __launch_bounds__(kMaxThreads) void ctc_beam_kernel(int T, int V, int K, const float* __restrict__ z, int64_t ld,
                                                               const int32_t* __restrict__ lens, int32_t* __restrict__ hyp,
                                                               int32_t* __restrict__ hyp_len, float* __restrict__ score,
                                                               BeamWs w) {
  __shared__ float s_pb[2][kKmax], s_pnb[2][kKmax], s_tot[2][kKmax];
  __shared__ int s_last[2][kKmax], s_len[2][kKmax];
  __shared__ u64 s_hash[2][kKmax];
  __shared__ unsigned s_mk[kKmax];                           // entry k: the entries that are prefix_k + one token
  __shared__ float s_spb[kKmax], s_spnb[kKmax];              // the stay candidate's (pb', pnb') of entry k
  __shared__ float xs[kStage * kMaxThreads];                 // x[t][c] of this frame, c < kStage * threads
  __shared__ float red_v[2][kMaxThreads / 64];
  __shared__ int red_i[2][kMaxThreads / 64];
  __shared__ int2 s_hist[kHistLds];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  const int len = clamp_len(lens[b], T);
  int32_t* hypb = hyp + (int64_t)b * K * T;
  if (len == 0) {                                            // no frames: the empty hypothesis at score 0
    for (int64_t i = tid; i < (int64_t)K * T; i += nt) hypb[i] = -1;
    if (tid < K) {
      score[(int64_t)b * K + tid] = tid == 0 ? 0.f : -INFINITY;
      hyp_len[(int64_t)b * K + tid] = tid == 0 ? 0 : -1;
    }
    return;
  }
  const float* zb = z + (int64_t)b * T * ld;
  const float* lse = w.lse + (int64_t)b * T;
  int2* hist = (int64_t)len * K <= kHistLds ? s_hist : w.hist + (int64_t)b * T * K;
  const int nstage = kStage * nt;
  if (tid < K) {                                             // the empty prefix at (0, -inf)
    s_pb[0][tid] = tid == 0 ? 0.f : -INFINITY;
    s_pnb[0][tid] = -INFINITY;
    s_tot[0][tid] = tid == 0 ? 0.f : -INFINITY;
    s_last[0][tid] = -1;
    s_len[0][tid] = 0;
    s_hash[0][tid] = 0;
  }
  float zn[kStage];
  float ln = lse[0];
#pragma unroll
  for (int i = 0; i < kStage; ++i) {
    const int c = tid + i * nt;
    zn[i] = c < V ? zb[c] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < kStage; ++i) xs[tid + i * nt] = zn[i] - ln;
  __syncthreads();
  int p = 0, nlive = 1;
  for (int t = 0; t < len; ++t) {
    const float* zr = zb + (int64_t)t * ld;
    const float lcur = ln;
    if (t + 1 < len) {                                       // the next frame's emissions: in flight while this frame runs
      ln = lse[t + 1];
#pragma unroll
      for (int i = 0; i < kStage; ++i) {
        const int c = tid + i * nt;
        if (c < V) zn[i] = zr[ld + c];
      }
    }
    // the merge map
    if (tid < nlive) {
      const u64 hj = s_hash[p][tid];
      const int lj = s_len[p][tid];
      unsigned mk = 0;
      for (int i = 0; i < nlive; ++i)
        if (s_len[p][i] == lj + 1 && prefix_hash(hj, s_last[p][i]) == s_hash[p][i]) mk |= 1u << i;
      s_mk[tid] = mk;
    }
    __syncthreads();
    float lv[M];
    int li[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
      lv[j] = -INFINITY;
      li[j] = INT_MAX;
    }
    // the stay candidate of entry tid (flat index tid: the lowest of this thread's candidates)
    if (tid < nlive) {
      const int cj = s_last[p][tid], lj = s_len[p][tid];
      const u64 hj = s_hash[p][tid];
      const float x0 = xs[0];
      const float xj = cj < 0 ? 0.f : (cj < nstage ? xs[cj] : zr[cj] - lcur);
      const float npb = s_tot[p][tid] + x0;
      float npnb = cj < 0 ? -INFINITY : s_pnb[p][tid] + xj;
      for (int i = 0; i < nlive; ++i)                        // prefix_i . cj is this entry: its mass joins here
        if (cj >= 0 && s_len[p][i] + 1 == lj && prefix_hash(s_hash[p][i], cj) == hj)
          npnb = logaddexp(npnb, (s_last[p][i] == cj ? s_pb[p][i] : s_tot[p][i]) + xj);
      s_spb[tid] = npb;
      s_spnb[tid] = npnb;
      top_insert(lv, li, logaddexp(npb, npnb), tid);
    }
    // the extensions, entry-major
    for (int k = 0; k < nlive; ++k) {
      const int ck = s_last[p][k];
      const float pbk = s_pb[p][k], totk = s_tot[p][k];
      const unsigned mkk = s_mk[k];
      const int base = K + k * (V - 1) - 1;
      for (int c = tid; c < V; c += nt) {
        if (c == 0) continue;
        const float xc = c < nstage ? xs[c] : zr[c] - lcur;
        float val = (c == ck ? pbk : totk) + xc;
        for (unsigned m = mkk; m; m &= m - 1)                // prefix_k . c is in the beam: not a candidate of its own
          if (s_last[p][__ffs(m) - 1] == c) val = -INFINITY;
        top_insert(lv, li, val, base + c);
      }
    }
    // select: K rounds of the workgroup arg-best over the list heads; the owner of the winner pops its head.  The list's clear
    // above, the round and the pop are seq_common.h's top_clear / top_round / top_pop_if_head spelled out: this loop runs K
    // times per frame on the serial chain, and through the helpers the compiler gives it another shape
    int nsel = 0, my_i = INT_MAX;
    float my_v = -INFINITY;
    for (int r = 0; r < K; ++r) {
      float v = lv[0];
      int i = li[0];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        if (better(ov, oi, v, i)) {
          v = ov;
          i = oi;
        }
      }
      if (nw > 1) {                                          // (uniform) double-buffered: one barrier per round
        const int buf = r & 1;
        if (lane == 0) {
          red_v[buf][wave] = v;
          red_i[buf][wave] = i;
        }
        __syncthreads();
        v = red_v[buf][0];
        i = red_i[buf][0];
        for (int ww = 1; ww < nw; ++ww)
          if (better(red_v[buf][ww], red_i[buf][ww], v, i)) {
            v = red_v[buf][ww];
            i = red_i[buf][ww];
          }
      }
      if (v == -INFINITY) break;                             // fewer than K candidates above -inf (uniform)
      if (li[0] == i) {
#pragma unroll
        for (int j = 0; j < M - 1; ++j) {
          lv[j] = lv[j + 1];
          li[j] = li[j + 1];
        }
        lv[M - 1] = -INFINITY;
        li[M - 1] = INT_MAX;
      }
      if (tid == r) {
        my_v = v;
        my_i = i;
      }
      nsel = r + 1;
    }
    __syncthreads();                                         // every read of xs and of slot p's candidates is done
    // update: entry tid of the other slot, and the frame's history
    const int q = p ^ 1;
    if (tid < K) {
      if (tid < nsel) {
        int k, tok;
        if (my_i < K) {
          k = my_i, tok = 0;
          s_pb[q][tid] = s_spb[k];
          s_pnb[q][tid] = s_spnb[k];
          s_last[q][tid] = s_last[p][k];
          s_len[q][tid] = s_len[p][k];
          s_hash[q][tid] = s_hash[p][k];
        } else {
          const int e = my_i - K;
          k = e / (V - 1), tok = e - k * (V - 1) + 1;
          s_pb[q][tid] = -INFINITY;
          s_pnb[q][tid] = my_v;
          s_last[q][tid] = tok;
          s_len[q][tid] = s_len[p][k] + 1;
          s_hash[q][tid] = prefix_hash(s_hash[p][k], tok);
        }
        s_tot[q][tid] = my_v;
        hist[(int64_t)t * K + tid] = make_int2(k, tok);
      } else {
        s_tot[q][tid] = -INFINITY;
      }
    }
    if (t + 1 < len) {
#pragma unroll
      for (int i = 0; i < kStage; ++i) xs[tid + i * nt] = zn[i] - ln;
    }
    __syncthreads();
    p = q;
    nlive = nsel;
  }
  // the beam is the ranking; thread r walks the history of entry r back into its row
  if (tid < K) {
    int32_t* row = hypb + (int64_t)tid * T;
    if (tid < nlive) {
      const int n = s_len[p][tid];
      int pos = n - 1, slot = tid;
      for (int t = len - 1; t >= 0; --t) {
        const int2 e = hist[(int64_t)t * K + slot];
        if (e.y != 0 && pos >= 0) row[pos--] = e.y;
        slot = e.x;
      }
      score[(int64_t)b * K + tid] = s_tot[p][tid];
      hyp_len[(int64_t)b * K + tid] = n;
    } else {
      score[(int64_t)b * K + tid] = -INFINITY;
      hyp_len[(int64_t)b * K + tid] = -1;
    }
  }
  for (int r = 0; r < K; ++r) {
    const int n = r < nlive ? s_len[p][r] : 0;
    for (int i = n + tid; i < T; i += nt) hypb[(int64_t)r * T + i] = -1;
  }
}

int beam_check(int B, int T, int V, int K) {
  if (B <= 0 || T <= 0 || V <= 0) return ASR_E_ARG;
  if (V < 2 || K < 1 || K > kKmax || (int64_t)K * V > INT_MAX / 2 || ((int64_t)B * T + kLseWaves - 1) / kLseWaves > 0x7fffffffLL)
    return ASR_E_SHAPE;
  return 0;
}

}  // namespace

extern "C" int asr_ctc_beam_ws_bytes(int B, int T, int V, int K, int64_t* ws_bytes) {
  if (!ws_bytes) return ASR_E_ARG;
  const int rc = beam_check(B, T, V, K);
  if (rc) return rc;
  *ws_bytes = beam_ws(nullptr, B, T, K).bytes;
  return 0;
}

extern "C" int asr_ctc_beam_f32(int B, int T, int V, int K, const float* logits, int64_t ld, const int32_t* frame_lens,
                                int32_t* hyp, int32_t* hyp_len, float* score, void* ws, asr_stream_t stream) {
  if (!logits || !frame_lens || !hyp || !hyp_len || !score || !ws || ld < V) return ASR_E_ARG;
  const int rc = beam_check(B, T, V, K);
  if (rc) return rc;
  if ((((uintptr_t)ws) & 7u) != 0) return ASR_E_ALIGN;
  const BeamWs w = beam_ws(ws, B, T, K);
  launch_frame_lse(B, T, V, logits, ld, frame_lens, w.lse, (hipStream_t)stream);
  ASR_CHECK_LAUNCH();
  const dim3 grid(B), block((int64_t)K * V <= kOneWaveKV ? 64 : kMaxThreads);
#define CTC_BEAM(M_) \
  hipLaunchKernelGGL((ctc_beam_kernel<M_>), grid, block, 0, (hipStream_t)stream, T, V, K, logits, ld, frame_lens, hyp, hyp_len, \
                     score, w)
  if (K <= 1) CTC_BEAM(1);
  else if (K <= 2) CTC_BEAM(2);
  else if (K <= 4) CTC_BEAM(4);
  else if (K <= 8) CTC_BEAM(8);
  else CTC_BEAM(16);
#undef CTC_BEAM
  ASR_CHECK_LAUNCH();
  return 0;
}
