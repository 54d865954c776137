// ctc_prefix.hip — the CTC prefix score of joint CTC-attention beam search (Watanabe et al. 2017) on the
// device.  Blank = <PAD> = index 0 by convention (the caller names it); x[t][v] = logits[b][t][v] - lse[b][t] and the valid
// frames of utterance b are seq_common.h's.  Every beam row carries r_n[t], r_b[t] - the log-probability of its prefix g ending at
// frame t in a non-blank / a blank - as (r_n, r_b) pairs [row][t][2] in two slots, its last token (-1: g is empty) and
// psi_prev = psi(g).  Three kernels, no atomics, every sum in an order fixed by the shapes:
//   ctc_prefix_init_kernel     one workgroup per utterance, once per search: lse[b][t] (a wave per frame), then wave 0 scans
//                              x[t][blank] into r_b (64 frames per round, Hillis-Steele inside the wave, the carry added
//                              behind it) and writes the empty prefix's state into slot 0 of the utterance's K rows
//   ctc_prefix_score_kernel    one wave per (beam row, 64 tokens): lanes are tokens, frames in sequence - a frame's logits
//                              are one coalesced read, r_n[t-1], r_b[t-1] and lse[t] are the same word for the whole wave;
//                              psi(g c) = logsumexp_t (phi[t-1] + x[t][c]) as a running (max, sum): one expf per frame and
//                              lane, no state per candidate
//   ctc_prefix_advance_kernel  one wave per beam row (a workgroup per utterance: its rows share the frames' blank and lse
//                              words through the cache): 64 frames per round - every lane loads its frame's x[t][c],
//                              x[t][blank] and the predecessor's phi[t-1] (the next round's loads are issued before this
//                              round's chain runs), then the n / b chain walks the 64 frames through readlane
#include <float.h>
#include "seq_common.h"

namespace {

// log(exp(a) + exp(b)); (-inf, -inf) -> -inf, never NaN for arguments below +inf
// (not seq_common.h's logaddexp: logf(1 + .) here, log1pf there - they round differently, and each search's bits are its own)
__device__ __forceinline__ float lae(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + logf(1.f + expf(-fabsf(a - b)));
}

__device__ __forceinline__ float lane_read(float v, int j) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j));
}

__global__ __launch_bounds__(256) void ctc_prefix_init_kernel(asr_ctc_prefix_t c) {
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int len = clamp_len(c.frame_lens[b], c.Tp), V = c.V, K = c.K;
  const float* zb = c.logits + (int64_t)b * c.Tp * c.ld;
  float* lse = c.lse + (int64_t)b * c.Tp;
  for (int t = wave; t < len; t += 4) {                        // frames behind the utterance are never read
    float mx, se;
    wave_row_max_sumexp(zb + (int64_t)t * c.ld, V, lane, mx, se);
    if (lane == 0) lse[t] = mx + logf(se);
  }
  __syncthreads();
  if (wave != 0) return;
  for (int k = lane; k < K; k += 64) {
    c.last[0][b * K + k] = -1;
    c.psi_prev[b * K + k] = 0.f;
  }
  float carry = 0.f;
  for (int t0 = 0; t0 < len; t0 += 64) {
    const int t = t0 + lane;
    float v = t < len ? zb[(int64_t)t * c.ld + c.blank] - lse[t] : 0.f;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float u = __shfl_up(v, off, 64);
      if (lane >= off) v += u;
    }
    v += carry;
    carry = lane_read(v, 63);
    if (t < len)
      for (int k = 0; k < K; ++k)
        reinterpret_cast<float2*>(c.state[0])[((int64_t)b * K + k) * c.Tp + t] = make_float2(-INFINITY, v);
  }
}

__global__ __launch_bounds__(64) void ctc_prefix_score_kernel(asr_ctc_prefix_t c, const float* __restrict__ scores,
                                                              const int32_t* __restrict__ done, int slot) {
  const int row = blockIdx.y, b = row / c.K, lane = threadIdx.x;
  if (done[b] || scores[row] == -INFINITY) return;            // dead rows and done utterances: psi is left as it is
  const int v = blockIdx.x * 64 + lane, V = c.V;
  const int len = clamp_len(c.frame_lens[b], c.Tp);
  if (len < 1) {                                                // no frame: nothing can be emitted
    if (v < V) c.psi[(int64_t)row * V + v] = -INFINITY;
    return;
  }
  const int vv = v < V ? v : V - 1;                             // lanes behind V read a valid word and store nothing
  const float* zb = c.logits + (int64_t)b * c.Tp * c.ld + vv;
  const float* lse = c.lse + (int64_t)b * c.Tp;
  const float2* r = reinterpret_cast<const float2*>(c.state[slot]) + (int64_t)row * c.Tp;
  const int last = c.last[slot][row];
  const bool same = vv == last;
  // running log-sum-exp (m, s): the sum is s * exp(m)
  float m = last < 0 ? zb[0] - lse[0] : -INFINITY;              // p0 = x[0][c] for the empty prefix
  float s = m == -INFINITY ? 0.f : 1.f;
#pragma unroll 4
  for (int t = 1; t < len; ++t) {
    const float2 p = r[t - 1];
    const float phi = same ? p.y : lae(p.x, p.y);
    const float a = phi + (zb[(int64_t)t * c.ld] - lse[t]);
    // one expf per frame, no branch: e is NaN only where a and m are both -inf, and then a is skipped
    const float e = expf(-fabsf(a - m));
    const bool up = a > m;
    const float ns = up ? s * e + 1.f : s + e;
    s = a == -INFINITY ? s : ns;
    m = up ? a : m;
  }
  float psi = m == -INFINITY ? -INFINITY : m + logf(s);
  if (vv == c.eos) psi = lae(r[len - 1].x, r[len - 1].y);
  if (vv == c.blank) psi = -INFINITY;
  if (v < V) c.psi[(int64_t)row * V + v] = psi;
}

__global__ __launch_bounds__(1024) void ctc_prefix_advance_kernel(asr_ctc_prefix_t c, asr_beam_t p, int t, int src_slot,
                                                                 int dst_slot) {
  const int b = blockIdx.x, lane = threadIdx.x & 63, j = threadIdx.x >> 6, K = c.K;
  const int row = b * K + j;
  if (p.done[b] || p.scores[row] == -INFINITY) return;         // done utterances and dead slots are left untouched
  const int64_t h = ((int64_t)t * p.B + b) * K + j;
  const int src = b * K + p.bp_hist[h], tok = p.tok_hist[h];
  const int len = clamp_len(c.frame_lens[b], c.Tp);
  const int last = c.last[src_slot][src];
  const bool same = tok == last;
  const float* zb = c.logits + (int64_t)b * c.Tp * c.ld;
  const float* lse = c.lse + (int64_t)b * c.Tp;
  const float2* rs = reinterpret_cast<const float2*>(c.state[src_slot]) + (int64_t)src * c.Tp;
  float2* rd = reinterpret_cast<float2*>(c.state[dst_slot]) + (int64_t)row * c.Tp;
  if (lane == 0) {
    c.psi_prev[row] = c.psi[(int64_t)src * c.V + tok];
    c.last[dst_slot][row] = tok;
  }
  if (len < 1) return;
  float n = last < 0 ? zb[tok] - lse[0] : -INFINITY, bl = -INFINITY;
  if (lane == 0) rd[0] = make_float2(n, bl);
  // this round's frames t0 + lane: the candidate's and the blank's log-probability, the predecessor's state one frame back
  float xc = 0.f, x0 = 0.f, l = 0.f;
  float2 pr = make_float2(-INFINITY, -INFINITY);
  if (1 + lane < len) {
    const int f = 1 + lane;
    xc = zb[(int64_t)f * c.ld + tok], x0 = zb[(int64_t)f * c.ld + c.blank], l = lse[f], pr = rs[f - 1];
  }
  for (int t0 = 1; t0 < len; t0 += 64) {
    const float cxc = xc - l, cx0 = x0 - l;
    const float phi = same ? pr.y : lae(pr.x, pr.y);
    const int f = t0 + 64 + lane;                               // the next round's loads, in flight over the chain
    if (f < len) xc = zb[(int64_t)f * c.ld + tok], x0 = zb[(int64_t)f * c.ld + c.blank], l = lse[f], pr = rs[f - 1];
    const int cnt = len - t0 < 64 ? len - t0 : 64;
    float on = -INFINITY, ob = -INFINITY;
    for (int i = 0; i < cnt; ++i) {
      const float nn = lae(n, lane_read(phi, i)) + lane_read(cxc, i);
      bl = lae(n, bl) + lane_read(cx0, i);
      n = nn;
      if (lane == i) on = n, ob = bl;
    }
    if (t0 + lane < len) rd[t0 + lane] = make_float2(on, ob);
  }
}

int check_prefix(const asr_ctc_prefix_t* c) {
  if (!c || !c->logits || !c->frame_lens || !c->lse || !c->state[0] || !c->state[1] || !c->last[0] || !c->last[1] || !c->psi ||
      !c->psi_prev)
    return ASR_E_ARG;
  if (c->B <= 0 || c->K <= 0 || c->Tp <= 0 || c->ld < c->V) return ASR_E_ARG;
  if (c->state[0] == c->state[1] || c->last[0] == c->last[1]) return ASR_E_ARG;      // the advance is out of place
  if (c->K > ASR_BEAM_KMAX || c->V < 3 || c->eos < 0 || c->eos >= c->V || c->blank < 0 || c->blank >= c->V || c->eos == c->blank ||
      (int64_t)c->B * c->K > 65535)
    return ASR_E_SHAPE;
  if ((((uintptr_t)c->state[0]) | ((uintptr_t)c->state[1])) & 7u) return ASR_E_ALIGN;      // (r_n, r_b) pairs: 8 bytes
  return 0;
}

int check_pair(const asr_ctc_prefix_t* c, const asr_beam_t* p) {
  int rc = check_prefix(c);
  if (rc) return rc;
  if (!p || !p->scores || !p->done || !p->tok_hist || !p->bp_hist) return ASR_E_ARG;
  if (p->B != c->B || p->K != c->K || p->V != c->V || p->eos != c->eos) return ASR_E_ARG;
  return 0;
}

}  // namespace

extern "C" int asr_ctc_prefix_init_f32(const asr_ctc_prefix_t* c, const int32_t* host_lens, asr_stream_t stream_) {
  int rc = check_prefix(c);
  if (rc) return rc;
  if (host_lens)                                                // the caller's host copy of frame_lens, where it has one
    for (int b = 0; b < c->B; ++b)
      if (host_lens[b] < 1 || host_lens[b] > c->Tp) return ASR_E_SHAPE;
  hipLaunchKernelGGL(ctc_prefix_init_kernel, dim3(c->B), dim3(256), 0, (hipStream_t)stream_, *c);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_ctc_prefix_score_f32(const asr_ctc_prefix_t* c, const asr_beam_t* p, int slot, asr_stream_t stream_) {
  int rc = check_pair(c, p);
  if (rc) return rc;
  if (slot != 0 && slot != 1) return ASR_E_ARG;
  hipLaunchKernelGGL(ctc_prefix_score_kernel, dim3((c->V + 63) / 64, c->B * c->K), dim3(64), 0, (hipStream_t)stream_, *c,
                     p->scores, p->done, slot);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_ctc_prefix_advance_f32(const asr_ctc_prefix_t* c, const asr_beam_t* p, int t, int src_slot, int dst_slot,
                                          asr_stream_t stream_) {
  int rc = check_pair(c, p);
  if (rc) return rc;
  if (t < 0 || t >= p->L || (src_slot != 0 && src_slot != 1) || (dst_slot != 0 && dst_slot != 1)) return ASR_E_ARG;
  if (src_slot == dst_slot) return ASR_E_ARG;                   // a gather over the beams: out of place
  hipLaunchKernelGGL(ctc_prefix_advance_kernel, dim3(c->B), dim3(64 * c->K), 0, (hipStream_t)stream_, *c, *p, t, src_slot,
                     dst_slot);
  ASR_CHECK_LAUNCH();
  return 0;
}
