// ctc_align.hip — the Viterbi (max-product) companions of ctc.hip on the CTC head's logits: forced alignment of a transcript
// and best-path (greedy) decoding.  The conventions are seq_common.h's; its frame_lse_kernel runs first.
//   ctc_align_kernel      one workgroup per utterance (one wave when max S <= 64, states strided over 256 threads above 256
//                         states).  Four phases in one launch:
//                           chain      v over the frames with max in place of logsumexp - adds and compares only; two rows of
//                                      LDS, one barrier per frame, the emissions of the two frames ahead in flight.  Each
//                                      state's choice (0 stay, 1 from s-1, 2 from s-2; strictly-greater replaces, in that
//                                      order) is two bits: two wave ballots per frame give a pair of 64-bit words per
//                                      (frame, 64 states), written by one lane - to LDS when T_b ceil(S / 64) 16 bytes fit
//                                      kBpLdsBytes, to the workspace otherwise
//                           backtrace  one lane walks the T_b frames down from the better end state and writes the state
//                                      of every frame
//                           output     parallel over the frames: path, and first / last of the label whose run starts /
//                                      ends at the frame
//                           sums       parallel over the labels: token_logp, by one lane in ascending frame order
//   ctc_greedy_kernel     one workgroup per utterance: a wave takes a frame's argmax over the raw logits (NaN never wins,
//                         ties to the lowest index); then one wave compacts the kept frames (non-blank, not a repeat of the
//                         frame before) in frame order by ballot and popcount
#include "seq_common.h"

namespace {

constexpr int kBpLdsBytes = ASR_CTC_ALIGN_LDS_BYTES;      // the back-pointers of an utterance stay in LDS up to this size
constexpr int kBpLdsWords = kBpLdsBytes / 8;
static_assert(kBpLdsBytes % 16 == 0, "a (frame, 64 states) entry is a pair of 64-bit words");
static_assert(kBpLdsBytes + 2 * (kMaxS + 5) * 4 + (kMaxL + 1) * 4 + 64 <= 64 * 1024, "the static LDS of a workgroup");

typedef unsigned long long u64;

struct AlignWs {
  float* lse;      // [B][T]
  int* state;      // [B][T]              the state of every frame (the backtrace's output)
  u64* bp;         // [B][T][nwp][2]      back-pointer words; nwp = ceil((2 max_label_len + 1) / 64); absent when they fit LDS
  int64_t bytes;
};

AlignWs align_ws(void* base, int B, int T, int Lmax) {
  const int64_t nwp = (2 * (int64_t)Lmax + 1 + 63) / 64;
  const int64_t n_bt = round64((int64_t)B * T);
  const int64_t n_bp = (int64_t)T * nwp * 16 > kBpLdsBytes ? (int64_t)B * T * nwp * 2 : 0;
  AlignWs w;
  w.bp = (u64*)base;                                       // (first: 8-byte aligned wherever the workspace is)
  w.lse = (float*)(w.bp + n_bp);
  w.state = (int*)(w.lse + n_bt);
  w.bytes = 8 * n_bp + 4 * 2 * n_bt;
  return w;
}

template <int NS>
__global__ __launch_bounds__(256) void ctc_align_kernel(int T, int V, const float* __restrict__ z, int64_t ld,
                                                        const int32_t* __restrict__ lens,
                                                        const int64_t* __restrict__ labels,
                                                        const int32_t* __restrict__ offs, int Lmax,
                                                        int32_t* __restrict__ path, float* __restrict__ score,
                                                        int32_t* __restrict__ first, int32_t* __restrict__ last,
                                                        float* __restrict__ token_logp, AlignWs w) {
  __shared__ float buf[2][kMaxS + 5];          // v of the previous / this frame at [s + 2]; [0], [1] stay -inf
  __shared__ int lab[kMaxL + 1];
  __shared__ u64 bpl[kBpLdsWords];
  __shared__ int bad, feasible;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int o0 = offs[b], L = offs[b + 1] - o0, S = 2 * L + 1;
  const int len = clamp_len(lens[b], T);
  int32_t* pathb = path + (int64_t)b * T;
  for (int i = tid; i < 2 * (kMaxS + 5); i += nt) (&buf[0][0])[i] = -INFINITY;
  // the labels into LDS; a label outside [1, V) or more labels than the launch was sized for: no alignment
  // (seq_common.h's ctc_load_labels with both barriers always taken: this kernel's code keeps that shape)
  if (tid == 0) bad = (L < 0 || L > Lmax) ? 1 : 0;
  __syncthreads();
  if (!bad) {
    for (int i = tid; i < L; i += nt) {
      const int64_t v = labels[o0 + i];
      if (v < 1 || v >= V) atomicOr(&bad, 1);
      lab[i] = (v < 1 || v >= V) ? 1 : (int)v;
    }
  }
  __syncthreads();
  if (bad || len == 0) {
    for (int t = tid; t < T; t += nt) pathb[t] = -1;
    for (int i = tid; i < L; i += nt) {
      first[o0 + i] = -1;
      last[o0 + i] = -1;
      token_logp[o0 + i] = -INFINITY;
    }
    if (tid == 0) score[b] = -INFINITY;
    return;
  }
  const int nw = (S + 63) >> 6;                              // 64-state words per frame
  const int nwp = (2 * Lmax + 1 + 63) >> 6;
  u64* bp = (int64_t)len * nw * 16 <= kBpLdsBytes ? bpl : w.bp + (int64_t)b * T * nwp * 2;
  const float* zb = z + (int64_t)b * T * ld;
  const float* lse = w.lse + (int64_t)b * T;
  int* st = w.state + (int64_t)b * T;
  int li[NS];
  bool act[NS], skip[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int s = tid + i * nt;
    act[i] = s < S;
    li[i] = (act[i] && (s & 1)) ? lab[s >> 1] : 0;
    skip[i] = act[i] && (s & 1) && s >= 3 && lab[s >> 1] != lab[(s >> 1) - 1];
  }
  // emissions of frames t, t + 1, t + 2 (raw logit; the frame's lse is subtracted where it is used)
  float z0[NS], z1[NS], z2[NS];
  float l0 = lse[0], l1 = len > 1 ? lse[1] : 0.f, l2 = 0.f;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    z0[i] = act[i] ? zb[li[i]] : 0.f;
    z1[i] = (act[i] && len > 1) ? zb[ld + li[i]] : 0.f;
    z2[i] = 0.f;
  }
  int p = 0;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int s = tid + i * nt;
    if (act[i]) buf[0][s + 2] = s < 2 ? z0[i] - l0 : -INFINITY;
  }
  __syncthreads();
  for (int t = 1; t < len; ++t) {
    if (t + 1 < len) {
      l2 = lse[t + 1];
#pragma unroll
      for (int i = 0; i < NS; ++i)
        if (act[i]) z2[i] = zb[(int64_t)(t + 1) * ld + li[i]];
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int s = tid + i * nt;
      int c = 0;
      if (act[i]) {
        const float a0 = buf[p][s + 2], a1 = buf[p][s + 1], a2 = skip[i] ? buf[p][s] : -INFINITY;
        float best = a0;
        if (a1 > best) { best = a1; c = 1; }
        if (a2 > best) { best = a2; c = 2; }
        buf[p ^ 1][s + 2] = best + (z1[i] - l1);
      }
      const u64 lo = __ballot(c & 1), hi = __ballot(c >> 1);
      const int word = wave + i * (nt >> 6);                 // the wave's 64 states of this round
      if (lane == 0 && word < nw) {
        u64* e = bp + ((int64_t)t * nw + word) * 2;
        e[0] = lo;
        e[1] = hi;
      }
    }
    __syncthreads();
    p ^= 1;
    l1 = l2;
#pragma unroll
    for (int i = 0; i < NS; ++i) z1[i] = z2[i];
  }
  // the backtrace: S - 1 unless S - 2 is strictly greater, then the stored choices down to frame 0
  if (tid == 0) {
    const float e1 = buf[p][S - 1 + 2], e2 = S > 1 ? buf[p][S - 2 + 2] : -INFINITY;
    int s = e2 > e1 ? S - 2 : S - 1;
    const float best = e2 > e1 ? e2 : e1;
    const int ok = best > -INFINITY;
    feasible = ok;
    score[b] = ok ? best : -INFINITY;
    if (ok) {
      for (int t = len - 1; t >= 1; --t) {
        st[t] = s;
        const u64* e = bp + ((int64_t)t * nw + (s >> 6)) * 2;
        const int c = (int)((e[0] >> (s & 63)) & 1) | ((int)((e[1] >> (s & 63)) & 1) << 1);
        s -= c;
      }
      st[0] = s;
    }
  }
  __syncthreads();
  if (!feasible) {
    for (int t = tid; t < T; t += nt) pathb[t] = -1;
    for (int i = tid; i < L; i += nt) {
      first[o0 + i] = -1;
      last[o0 + i] = -1;
      token_logp[o0 + i] = -INFINITY;
    }
    return;
  }
  // the token of every frame; the frame where a label's run starts / ends (each label has exactly one of either)
  for (int t = tid; t < T; t += nt) {
    if (t >= len) {
      pathb[t] = -1;
      continue;
    }
    const int s = st[t];
    pathb[t] = (s & 1) ? lab[s >> 1] : 0;
    if (s & 1) {
      if (t == 0 || st[t - 1] != s) first[o0 + (s >> 1)] = t;
      if (t == len - 1 || st[t + 1] != s) last[o0 + (s >> 1)] = t;
    }
  }
  __syncthreads();
  for (int i = tid; i < L; i += nt) {
    const int f = first[o0 + i], l = last[o0 + i], k = lab[i];
    float sum = 0.f;
    for (int t = f < 0 ? 0 : f; t <= l && t < len; ++t) sum += zb[(int64_t)t * ld + k] - lse[t];    // (0 <= f <= l < len)
    token_logp[o0 + i] = sum;
  }
}

__global__ __launch_bounds__(256) void ctc_greedy_kernel(int T, int V, const float* __restrict__ z, int64_t ld,
                                                         const int32_t* __restrict__ lens, int32_t* __restrict__ ids,
                                                         int32_t* __restrict__ n, int32_t* __restrict__ frame_tok) {
  __shared__ int kept_total;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int len = clamp_len(lens[b], T);
  const float* zb = z + (int64_t)b * T * ld;
  int32_t* ft = frame_tok + (int64_t)b * T;
  int32_t* idb = ids + (int64_t)b * T;
  for (int t = wave; t < T; t += 4) {
    if (t >= len) {                                          // (wave-uniform)
      if (lane == 0) ft[t] = -1;
      continue;
    }
    const float* zr = zb + (int64_t)t * ld;
    float best = -INFINITY;
    int bi = lane < V ? lane : 0x7fffffff;
    for (int v = lane; v < V; v += 64) {
      const float x = zr[v];
      if (x > best) {                                        // (false for NaN; ascending v: the first of equal values stays)
        best = x;
        bi = v;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ob = __shfl_xor(best, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (ob > best || (ob == best && oi < bi)) {
        best = ob;
        bi = oi;
      }
    }
    if (lane == 0) ft[t] = bi;
  }
  __syncthreads();
  if (wave == 0) {
    int count = 0;
    for (int t0 = 0; t0 < len; t0 += 64) {
      const int t = t0 + lane;
      const int a = t < len ? ft[t] : 0;
      const int prev = (t < len && t > 0) ? ft[t - 1] : 0;
      const bool keep = t < len && a != 0 && (t == 0 || a != prev);
      const u64 kept = __ballot(keep);
      if (keep) idb[count + __popcll(kept & ((1ull << lane) - 1ull))] = a;
      count += __popcll(kept);
    }
    if (lane == 0) {
      kept_total = count;
      n[b] = count;
    }
  }
  __syncthreads();
  for (int t = kept_total + tid; t < T; t += 256) idb[t] = -1;
}

}  // namespace

extern "C" int asr_ctc_align_ws_bytes(int B, int T, int V, int max_label_len, int64_t* ws_bytes) {
  if (!ws_bytes) return ASR_E_ARG;
  const int rc = ctc_shape_check(B, T, V, max_label_len);
  if (rc) return rc;
  *ws_bytes = align_ws(nullptr, B, T, max_label_len).bytes;
  return 0;
}

extern "C" int asr_ctc_align_f32(int B, int T, int V, const float* logits, int64_t ld, const int32_t* frame_lens,
                                 const int64_t* labels, const int32_t* label_offsets, int max_label_len, int32_t* path,
                                 float* score, int32_t* first, int32_t* last, float* token_logp, void* ws, int64_t ws_bytes,
                                 asr_stream_t stream) {
  if (!logits || !frame_lens || !label_offsets || !path || !score || !ws || ld < V) return ASR_E_ARG;
  if (max_label_len > 0 && (!labels || !first || !last || !token_logp)) return ASR_E_ARG;
  const int rc = ctc_shape_check(B, T, V, max_label_len);
  if (rc) return rc;
  if ((((uintptr_t)ws) & 7u) != 0) return ASR_E_ALIGN;
  const AlignWs w = align_ws(ws, B, T, max_label_len);
  if (ws_bytes < w.bytes) return ASR_E_ARG;
  launch_frame_lse(B, T, V, logits, ld, frame_lens, w.lse, (hipStream_t)stream);
  ASR_CHECK_LAUNCH();
  launch_by_states(2 * max_label_len + 1, ctc_align_kernel<1>, ctc_align_kernel<8>, B, (hipStream_t)stream, T, V, logits, ld,
                   frame_lens, labels, label_offsets, max_label_len, path, score, first, last, token_logp, w);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_ctc_greedy_f32(int B, int T, int V, const float* logits, int64_t ld, const int32_t* frame_lens,
                                  int32_t* ids, int32_t* n, int32_t* frame_tok, asr_stream_t stream) {
  if (!logits || !frame_lens || !ids || !n || !frame_tok || B <= 0 || T <= 0 || V <= 0 || ld < V) return ASR_E_ARG;
  if (V < 2) return ASR_E_SHAPE;
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, T, V, logits, ld, frame_lens, ids, n,
                     frame_tok);
  ASR_CHECK_LAUNCH();
  return 0;
}
