// ctc.hip — CTC loss on the encoder output (the CTC branch of joint CTC-attention training), forward and backward.
// The conventions (blank, extended labels, x = z - lse, ordered sums) are seq_common.h's; alpha / beta are kept in log space.
// Behind seq_common.h's frame_lse_kernel (the log-softmax lives in that one number per frame) three kernels:
//   ctc_alpha_kernel  one workgroup per utterance (one wave when max S <= 64): the label-sorted position list of the
//                     utterance (once), then alpha over the frames - states across threads (strided when S exceeds the
//                     workgroup), frames in sequence, the hand-off between frames through two rows of LDS with one barrier
//                     per frame; the emissions of the frames ahead are already in flight (two frames of register prefetch)
//   ctc_beta_kernel   the same chain backwards; writes alpha_t(s) + beta_t(s) over alpha_t(s)
//   ctc_grad_kernel   one wave per frame: the blank's states are summed by the whole wave, every other vocabulary entry by
//                     the lane that owns it, walking its run of the sorted position list in ascending order
#include "seq_common.h"

namespace {

constexpr int kHeadShift = 12;                 // head entry = (first index in the sorted list << 12) | run length; 0: absent
static_assert(kMaxL < (1 << kHeadShift), "the run length must fit the low bits of a head entry");

struct CtcWs {
  float* lse;      // [B][T]
  float* raw;      // [B]            the nll before zero_infinity
  float* ab;       // [B][T][Sp]     alpha, after the backward's first kernel alpha + beta;  Sp = 2 max_label_len + 1
  int* order;      // [B][Lo]        label positions sorted by (label, position);            Lo = max(max_label_len, 1)
  int* head;       // [B][V]
  int64_t bytes;
};

CtcWs ctc_ws(void* base, int B, int T, int V, int Lmax) {
  const int64_t Sp = 2 * (int64_t)Lmax + 1, Lo = Lmax > 0 ? Lmax : 1;
  const int64_t n_lse = round64((int64_t)B * T), n_raw = round64(B), n_ab = round64((int64_t)B * T * Sp),
                n_order = round64((int64_t)B * Lo), n_head = round64((int64_t)B * V);
  CtcWs w;
  float* f = (float*)base;
  w.lse = f;
  w.raw = w.lse + n_lse;
  w.ab = w.raw + n_raw;
  w.order = (int*)(w.ab + n_ab);
  w.head = w.order + n_order;
  w.bytes = 4 * (n_lse + n_raw + n_ab + n_order + n_head);
  return w;
}

__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  if (m == -INFINITY) return -INFINITY;
  return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}

template <int NS>
__global__ __launch_bounds__(256) void ctc_alpha_kernel(int T, int V, const float* __restrict__ z, int64_t ld,
                                                        const int32_t* __restrict__ lens,
                                                        const int64_t* __restrict__ labels,
                                                        const int32_t* __restrict__ offs, int Lmax, int zero_inf,
                                                        float* __restrict__ nll, CtcWs w) {
  __shared__ float buf[2][kMaxS + 5];          // alpha of the previous / this frame at [s + 2]; [0], [1] stay -inf
  __shared__ int lab[kMaxL + 1];
  __shared__ int bad;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int o0 = offs[b], L = offs[b + 1] - o0, S = 2 * L + 1;
  const int Sp = 2 * Lmax + 1, Lo = Lmax > 0 ? Lmax : 1;
  const int len = clamp_len(lens[b], T);
  for (int k = tid; k < V; k += nt) w.head[(int64_t)b * V + k] = 0;
  for (int i = tid; i < 2 * (kMaxS + 5); i += nt) (&buf[0][0])[i] = -INFINITY;
  const bool ok = ctc_load_labels(labels, o0, L, Lmax, V, lab, &bad);      // (its barriers order the fills above)
  if (!ok || len == 0) {
    if (tid == 0) {
      const float r = (ok && L == 0) ? 0.f : INFINITY;
      w.raw[b] = r;
      nll[b] = (zero_inf && r == INFINITY) ? 0.f : r;
    }
    return;
  }
  // the sorted position list: position i goes to rank #{j : (lab_j, j) < (lab_i, i)}; the first position of a label
  // records where its run starts and how long it is
  for (int i = tid; i < L; i += nt) {
    const int li = lab[i];
    int less = 0, eq_before = 0, eq = 0;
    for (int j = 0; j < L; ++j) {
      const int lj = lab[j];
      less += lj < li;
      eq += lj == li;
      eq_before += (lj == li) & (j < i);
    }
    const int r = less + eq_before;
    w.order[(int64_t)b * Lo + r] = i;
    if (eq_before == 0) w.head[(int64_t)b * V + li] = (r << kHeadShift) | eq;
  }
  const float* zb = z + (int64_t)b * T * ld;
  const float* lse = w.lse + (int64_t)b * T;
  float* ab = w.ab + (int64_t)b * T * Sp;
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
    if (act[i]) {
      const float a = s < 2 ? z0[i] - l0 : -INFINITY;
      buf[0][s + 2] = a;
      ab[s] = a;
    }
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
      if (act[i]) {
        const float a0 = buf[p][s + 2], a1 = buf[p][s + 1], a2 = skip[i] ? buf[p][s] : -INFINITY;
        const float a = lse3(a0, a1, a2) + (z1[i] - l1);
        buf[p ^ 1][s + 2] = a;
        ab[(int64_t)t * Sp + s] = a;
      }
    }
    __syncthreads();
    p ^= 1;
    l1 = l2;
#pragma unroll
    for (int i = 0; i < NS; ++i) z1[i] = z2[i];
  }
  if (tid == 0) {
    const float r = -lse3(buf[p][S - 1 + 2], S > 1 ? buf[p][S - 2 + 2] : -INFINITY, -INFINITY);
    w.raw[b] = r;
    nll[b] = (zero_inf && !(r < INFINITY)) ? 0.f : r;
  }
}

template <int NS>
__global__ __launch_bounds__(256) void ctc_beta_kernel(int T, int V, const float* __restrict__ z, int64_t ld,
                                                       const int32_t* __restrict__ lens,
                                                       const int64_t* __restrict__ labels,
                                                       const int32_t* __restrict__ offs, int Lmax, CtcWs w) {
  __shared__ float buf[2][kMaxS + 5];          // beta of the next / this frame at [s]; everything from [S] on stays -inf
  __shared__ int lab[kMaxL + 1];
  __shared__ int bad;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  if (!(w.raw[b] < INFINITY)) return;          // infeasible: the gradient kernel does not read alpha + beta
  const int o0 = offs[b], L = offs[b + 1] - o0, S = 2 * L + 1;
  const int Sp = 2 * Lmax + 1;
  const int len = clamp_len(lens[b], T);
  for (int i = tid; i < 2 * (kMaxS + 5); i += nt) (&buf[0][0])[i] = -INFINITY;
  if (!ctc_load_labels(labels, o0, L, Lmax, V, lab, &bad) || len == 0) return;
  const float* zb = z + (int64_t)b * T * ld;
  const float* lse = w.lse + (int64_t)b * T;
  float* ab = w.ab + (int64_t)b * T * Sp;
  int li[NS];
  bool act[NS], skip[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int s = tid + i * nt;
    act[i] = s < S;
    li[i] = (act[i] && (s & 1)) ? lab[s >> 1] : 0;
    skip[i] = act[i] && (s & 1) && s + 2 < S && lab[s >> 1] != lab[(s >> 1) + 1];
  }
  // emissions and alpha of frames t, t - 1, t - 2
  float z0[NS], z1[NS], z2[NS], a0[NS], a1[NS], a2[NS];
  int t = len - 1;
  float l0 = lse[t], l1 = t > 0 ? lse[t - 1] : 0.f, l2 = 0.f;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int s = tid + i * nt;
    z0[i] = act[i] ? zb[(int64_t)t * ld + li[i]] : 0.f;
    a0[i] = act[i] ? ab[(int64_t)t * Sp + s] : 0.f;
    z1[i] = (act[i] && t > 0) ? zb[(int64_t)(t - 1) * ld + li[i]] : 0.f;
    a1[i] = (act[i] && t > 0) ? ab[(int64_t)(t - 1) * Sp + s] : 0.f;
    z2[i] = a2[i] = 0.f;
  }
  int p = 0;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int s = tid + i * nt;
    if (act[i]) {
      const float be = s >= S - 2 ? z0[i] - l0 : -INFINITY;
      buf[0][s] = be;
      ab[(int64_t)t * Sp + s] = a0[i] + be;
    }
  }
  __syncthreads();
  for (t = len - 2; t >= 0; --t) {
    if (t > 0) {
      l2 = lse[t - 1];
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const int s = tid + i * nt;
        if (act[i]) {
          z2[i] = zb[(int64_t)(t - 1) * ld + li[i]];
          a2[i] = ab[(int64_t)(t - 1) * Sp + s];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int s = tid + i * nt;
      if (act[i]) {
        const float b0 = buf[p][s], b1 = buf[p][s + 1], b2 = skip[i] ? buf[p][s + 2] : -INFINITY;
        const float be = lse3(b0, b1, b2) + (z1[i] - l1);
        buf[p ^ 1][s] = be;
        ab[(int64_t)t * Sp + s] = a1[i] + be;
      }
    }
    __syncthreads();
    p ^= 1;
    l1 = l2;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      z1[i] = z2[i];
      a1[i] = a2[i];
    }
  }
}

// dz[b][t][k] = g_b (softmax_k - exp(logsum_{s : l'_s = k} (alpha + beta)_t(s) - logp_k + nll_b)); zeros behind the utterance
__global__ __launch_bounds__(256) void ctc_grad_kernel(int B, int T, int V, const float* __restrict__ z, int64_t ld,
                                                       const int32_t* __restrict__ lens,
                                                       const int32_t* __restrict__ offs, int Lmax, int zero_inf,
                                                       const float* __restrict__ g, CtcWs w, float* __restrict__ dz,
                                                       int64_t lddz) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (int64_t)B * T) return;
  const int b = (int)(row / T), t = (int)(row % T);
  float* dzr = dz + row * lddz;
  const float nllb = w.raw[b];
  const bool feasible = nllb < INFINITY;
  if (t >= lens[b] || (!feasible && zero_inf)) {
    for (int k = lane; k < V; k += 64) dzr[k] = 0.f;
    return;
  }
  const float* zr = z + row * ld;
  const float ls = w.lse[row], gb = g[b];
  if (!feasible) {                                           // no alignment: only the softmax term is defined
    for (int k = lane; k < V; k += 64) dzr[k] = gb * expf(zr[k] - ls);
    return;
  }
  const int L = offs[b + 1] - offs[b];
  const int Sp = 2 * Lmax + 1, Lo = Lmax > 0 ? Lmax : 1;
  const float* abr = w.ab + row * Sp;
  const int* order = w.order + (int64_t)b * Lo;
  const int* head = w.head + (int64_t)b * V;
  // the blank owns states 0, 2, .., 2L: lane-strided in ascending order, then the xor butterfly
  float m = -INFINITY;
  for (int i = lane; i <= L; i += 64) m = fmaxf(m, abr[2 * i]);
  m = wave_max(m);
  float lblank = -INFINITY;
  if (m > -INFINITY) {                                       // (wave-uniform)
    float se = 0.f;
    for (int i = lane; i <= L; i += 64) se += expf(abr[2 * i] - m);
    lblank = m + logf(wave_sum(se));
  }
  for (int k = lane; k < V; k += 64) {
    const float lp = zr[k] - ls;
    float lsum = lblank;
    if (k > 0) {
      const int e = head[k], n = e & ((1 << kHeadShift) - 1), h = e >> kHeadShift;
      lsum = -INFINITY;
      if (n > 0) {
        float mk = -INFINITY;
        for (int j = 0; j < n; ++j) mk = fmaxf(mk, abr[2 * order[h + j] + 1]);
        if (mk > -INFINITY) {
          float se = 0.f;
          for (int j = 0; j < n; ++j) se += expf(abr[2 * order[h + j] + 1] - mk);
          lsum = mk + logf(se);
        }
      }
    }
    const float occ = lsum > -INFINITY ? expf(lsum - lp + nllb) : 0.f;
    dzr[k] = gb * (expf(lp) - occ);
  }
}

int ctc_check(int B, int T, int V, int64_t ld, int Lmax, const void* ws, int64_t ws_bytes) {
  const int rc = ctc_shape_check(B, T, V, Lmax);
  if (rc == ASR_E_ARG || ld < V || !ws) return ASR_E_ARG;
  if (rc) return rc;
  if (ws_bytes < ctc_ws(nullptr, B, T, V, Lmax).bytes) return ASR_E_ARG;
  return 0;
}

}  // namespace

extern "C" int asr_ctc_ws_bytes(int B, int T, int V, int max_label_len, int64_t* ws_bytes) {
  if (B <= 0 || T <= 0 || V <= 0 || max_label_len < 0 || !ws_bytes) return ASR_E_ARG;
  if (V < 2 || max_label_len > kMaxL) return ASR_E_SHAPE;
  *ws_bytes = ctc_ws(nullptr, B, T, V, max_label_len).bytes;
  return 0;
}

extern "C" int asr_ctc_loss_fwd(int B, int T, int V, const float* logits, int64_t ld, const int32_t* frame_lens,
                                const int64_t* labels, const int32_t* label_offsets, int max_label_len, int zero_infinity,
                                float* nll, void* ws, int64_t ws_bytes, asr_stream_t stream) {
  if (!logits || !frame_lens || !labels || !label_offsets || !nll) return ASR_E_ARG;
  const int rc = ctc_check(B, T, V, ld, max_label_len, ws, ws_bytes);
  if (rc) return rc;
  const CtcWs w = ctc_ws(ws, B, T, V, max_label_len);
  launch_frame_lse(B, T, V, logits, ld, frame_lens, w.lse, (hipStream_t)stream);
  ASR_CHECK_LAUNCH();
  launch_by_states(2 * max_label_len + 1, ctc_alpha_kernel<1>, ctc_alpha_kernel<8>, B, (hipStream_t)stream, T, V, logits, ld,
                   frame_lens, labels, label_offsets, max_label_len, zero_infinity, nll, w);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_ctc_loss_bwd(int B, int T, int V, const float* logits, int64_t ld, const int32_t* frame_lens,
                                const int64_t* labels, const int32_t* label_offsets, int max_label_len, int zero_infinity,
                                const float* grad_nll, void* ws, int64_t ws_bytes, float* dlogits, int64_t lddz,
                                asr_stream_t stream) {
  if (!logits || !frame_lens || !labels || !label_offsets || !grad_nll || !dlogits || lddz < V) return ASR_E_ARG;
  const int rc = ctc_check(B, T, V, ld, max_label_len, ws, ws_bytes);
  if (rc) return rc;
  const CtcWs w = ctc_ws(ws, B, T, V, max_label_len);
  launch_by_states(2 * max_label_len + 1, ctc_beta_kernel<1>, ctc_beta_kernel<8>, B, (hipStream_t)stream, T, V, logits, ld,
                   frame_lens, labels, label_offsets, max_label_len, w);
  ASR_CHECK_LAUNCH();
  const unsigned rows4 = (unsigned)(((int64_t)B * T + 3) / 4);
  hipLaunchKernelGGL(ctc_grad_kernel, dim3(rows4), dim3(256), 0, (hipStream_t)stream, B, T, V, logits, ld, frame_lens,
                     label_offsets, max_label_len, zero_infinity, grad_nll, w, dlogits, lddz);
  ASR_CHECK_LAUNCH();
  return 0;
}
