// rnnt.hip — the transducer (RNN-T) head: joint network, loss forward / backward, one step of greedy decoding.
// The conventions are seq_common.h's (blank = 0, x = z - lse, ordered sums, no floating-point atomics: the same bits in
// every run and every mode).  A node is (b, t, u): frame t < T_b of utterance b after u <= U_b labels; the node matrices are
// [B][T][U + 1][.] row-major, every offset 64-bit.  Nodes off an utterance's lattice (t >= T_b or u > U_b) are padding:
// never read, and written as exact zeros where a kernel owns the output.
//   rnnt_joint_fwd_kernel   a thread per four joint units: Z = tanh(PE[b][t] + PP[b][u])
//   rnnt_joint_bwd_kernel   dZ (1 - Z^2) summed over u (ascending) into dPE, over t (ascending) into dPP: a thread per four
//                           units of one output row, so every sum has one owner
//   rnnt_lse_kernel         one wave per node: lse = logsumexp_v z (the log-softmax lives in that one number per node)
//   rnnt_alpha_kernel       one workgroup per utterance (one wave up to 64 label positions, 256 threads beyond, positions
//                           strided over the workgroup above 256): alpha by anti-diagonals t + u = d, label positions across
//                           the threads, the hand-off between diagonals through two rows of LDS with one barrier each
//   rnnt_beta_kernel        the same chain from the far corner
//   rnnt_grad_kernel        one wave per node: the softmax row times the node's occupancy, minus the two transitions
//   rnnt_greedy_step_kernel one workgroup per utterance: tanh, the J x V product (a wave per vocabulary entry, lanes strided
//                           over J, the xor butterfly), the argmax (greater value first, LOWER INDEX on ties) and the state
#include "seq_common.h"

namespace {

constexpr int kMaxU = ASR_RNNT_MAX_LABELS;
constexpr int kGreedyLds = 64 * 1024;           // bytes of dynamic LDS the greedy step may ask for: (J + V) floats

struct RnntWs {
  float* lse;      // [B][T][U + 1]
  float* alpha;    // [B][T][U + 1]
  float* beta;     // [B][T][U + 1]
  float* logp;     // [B]            log P(y | x) = -nll; -inf: the utterance cannot be scored
  int64_t bytes;
};

RnntWs rnnt_ws(void* base, int B, int T, int U1) {
  const int64_t n_node = round64((int64_t)B * T * U1), n_b = round64(B);
  RnntWs w;
  w.lse = (float*)base;
  w.alpha = w.lse + n_node;
  w.beta = w.alpha + n_node;
  w.logp = w.beta + n_node;
  w.bytes = 4 * (3 * n_node + n_b);
  return w;
}

// The sizes the kernels cover.  Offsets are 64-bit; what bounds a call is its launch grids: a wave per node in workgroups
// of four, a thread per four units in workgroups of 256.
int rnnt_shape_check(int B, int T, int U, int J, int V) {
  if (B <= 0 || T <= 0 || U < 0 || J <= 0 || V <= 0) return ASR_E_ARG;
  if (V < 2 || (J & 3) || U > kMaxU) return ASR_E_SHAPE;
  const __int128 nodes = (__int128)B * T * (U + 1);
  const __int128 elems = nodes * (J > V ? J : V);
  if ((nodes + 3) / 4 > 0x7fffffffLL || elems > ((__int128)1 << 40)) return ASR_E_SHAPE;
  return 0;
}

__device__ __forceinline__ int clamp_labels(int L, int U) { return L < 0 ? 0 : (L > U ? U : L); }

__device__ __forceinline__ float logaddexp2f(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + logf(expf(a - m) + expf(b - m));
}

__device__ __forceinline__ void node_of(int64_t node, int T, int U1, int& b, int& t, int& u) {
  u = (int)(node % U1);
  const int64_t bt = node / U1;
  t = (int)(bt % T);
  b = (int)(bt / T);
}

__global__ __launch_bounds__(256) void rnnt_joint_fwd_kernel(int64_t total, int T, int U1, int J4,
                                                             const float4* __restrict__ pe, const float4* __restrict__ pp,
                                                             const int32_t* __restrict__ lens,
                                                             const int32_t* __restrict__ offs, float4* __restrict__ z) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int j = (int)(idx % J4);
  int b, t, u;
  node_of(idx / J4, T, U1, b, t, u);
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  if (t < clamp_len(lens[b], T) && u <= clamp_labels(offs[b + 1] - offs[b], U1 - 1)) {
    const float4 e = pe[((int64_t)b * T + t) * J4 + j], p = pp[((int64_t)b * U1 + u) * J4 + j];
    r = make_float4(tanhf(e.x + p.x), tanhf(e.y + p.y), tanhf(e.z + p.z), tanhf(e.w + p.w));
  }
  z[idx] = r;
}

__device__ __forceinline__ void joint_acc(float4& s, const float4 d, const float4 v) {
  s.x += d.x * (1.f - v.x * v.x);
  s.y += d.y * (1.f - v.y * v.y);
  s.z += d.z * (1.f - v.z * v.z);
  s.w += d.w * (1.f - v.w * v.w);
}

// rows [0, B T): dPE[b][t]; rows [B T, B T + B (U + 1)): dPP[b][u]
__global__ __launch_bounds__(256) void rnnt_joint_bwd_kernel(int B, int T, int U1, int J4, const float4* __restrict__ dz,
                                                             const float4* __restrict__ z, const int32_t* __restrict__ lens,
                                                             const int32_t* __restrict__ offs, float4* __restrict__ dpe,
                                                             float4* __restrict__ dpp) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n_pe = (int64_t)B * T * J4, n_pp = (int64_t)B * U1 * J4;
  if (idx >= n_pe + n_pp) return;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (idx < n_pe) {
    const int j = (int)(idx % J4);
    const int64_t bt = idx / J4;
    const int b = (int)(bt / T), t = (int)(bt % T);
    if (t < clamp_len(lens[b], T)) {
      const int L = clamp_labels(offs[b + 1] - offs[b], U1 - 1);
      const int64_t n0 = (bt * U1) * J4 + j;
      for (int u = 0; u <= L; ++u) joint_acc(s, dz[n0 + (int64_t)u * J4], z[n0 + (int64_t)u * J4]);
    }
    dpe[idx] = s;
  } else {
    const int64_t i = idx - n_pe;
    const int j = (int)(i % J4);
    const int64_t bu = i / J4;
    const int b = (int)(bu / U1), u = (int)(bu % U1);
    if (u <= clamp_labels(offs[b + 1] - offs[b], U1 - 1)) {
      const int len = clamp_len(lens[b], T);
      const int64_t n0 = (((int64_t)b * T) * U1 + u) * J4 + j, st = (int64_t)U1 * J4;
      for (int t = 0; t < len; ++t) joint_acc(s, dz[n0 + t * st], z[n0 + t * st]);
    }
    dpp[i] = s;
  }
}

__global__ __launch_bounds__(256) void rnnt_lse_kernel(int64_t nodes, int T, int U1, int V, const float* __restrict__ z,
                                                       int64_t ld, const int32_t* __restrict__ lens,
                                                       const int32_t* __restrict__ offs, float* __restrict__ lse) {
  const int lane = threadIdx.x & 63;
  const int64_t node = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (node >= nodes) return;
  int b, t, u;
  node_of(node, T, U1, b, t, u);
  if (t >= clamp_len(lens[b], T) || u > clamp_labels(offs[b + 1] - offs[b], U1 - 1)) return;     // padding is never read
  float mx, se;
  wave_row_max_sumexp(z + node * ld, V, lane, mx, se);
  if (lane == 0) lse[node] = mx + logf(se);
}

// alpha(0, 0) = 0; alpha(t, u) = logaddexp(alpha(t-1, u) + lp_blank(t-1, u), alpha(t, u-1) + lp_{y_u}(t, u-1))
__global__ __launch_bounds__(256) void rnnt_alpha_kernel(int T, int U1, int V, const float* __restrict__ z, int64_t ld,
                                                         const int32_t* __restrict__ lens,
                                                         const int64_t* __restrict__ labels,
                                                         const int32_t* __restrict__ offs, float* __restrict__ nll, RnntWs w) {
  __shared__ float buf[2][kMaxU + 2];          // alpha of the previous / this diagonal at [u + 1]
  __shared__ int lab[kMaxU + 1];
  __shared__ int bad;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int o0 = offs[b], L = offs[b + 1] - o0;
  const int len = clamp_len(lens[b], T);
  const bool ok = ctc_load_labels(labels, o0, L, U1 - 1, V, lab, &bad);
  if (!ok || len == 0) {                       // a label outside [1, V), more labels than the launch holds, no frame
    if (tid == 0) {
      nll[b] = INFINITY;
      w.logp[b] = -INFINITY;
    }
    return;
  }
  const int64_t base = (int64_t)b * T * U1;
  int p = 0;
  for (int d = 0; d < len + L; ++d) {
    const int ulo = d - (len - 1) > 0 ? d - (len - 1) : 0, uhi = d < L ? d : L;
    for (int u = ulo + tid; u <= uhi; u += nt) {
      const int t = d - u;
      float a = 0.f;
      if (d > 0) {
        float up = -INFINITY, left = -INFINITY;
        if (t > 0) {
          const int64_t n = base + (int64_t)(t - 1) * U1 + u;
          up = buf[p][u + 1] + (z[n * ld] - w.lse[n]);
        }
        if (u > 0) {
          const int64_t n = base + (int64_t)t * U1 + (u - 1);
          left = buf[p][u] + (z[n * ld + lab[u - 1]] - w.lse[n]);
        }
        a = logaddexp2f(up, left);
      }
      buf[p ^ 1][u + 1] = a;
      w.alpha[base + (int64_t)t * U1 + u] = a;
    }
    __syncthreads();
    p ^= 1;
  }
  if (tid == 0) {
    const int64_t n = base + (int64_t)(len - 1) * U1 + L;
    const float lp = buf[p][L + 1] + (z[n * ld] - w.lse[n]);
    nll[b] = -lp;
    w.logp[b] = lp;
  }
}

// beta(T_b-1, U_b) = lp_blank; beta(t, u) = logaddexp(beta(t+1, u) + lp_blank(t, u), beta(t, u+1) + lp_{y_{u+1}}(t, u))
__global__ __launch_bounds__(256) void rnnt_beta_kernel(int T, int U1, int V, const float* __restrict__ z, int64_t ld,
                                                        const int32_t* __restrict__ lens,
                                                        const int64_t* __restrict__ labels,
                                                        const int32_t* __restrict__ offs, RnntWs w) {
  __shared__ float buf[2][kMaxU + 2];          // beta of the next / this diagonal at [u]
  __shared__ int lab[kMaxU + 1];
  __shared__ int bad;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  if (!(w.logp[b] > -INFINITY)) return;        // not scored: the gradient kernel writes zeros without reading beta
  const int o0 = offs[b], L = offs[b + 1] - o0;
  const int len = clamp_len(lens[b], T);
  if (!ctc_load_labels(labels, o0, L, U1 - 1, V, lab, &bad) || len == 0) return;
  const int64_t base = (int64_t)b * T * U1;
  int p = 0;
  for (int d = len - 1 + L; d >= 0; --d) {
    const int ulo = d - (len - 1) > 0 ? d - (len - 1) : 0, uhi = d < L ? d : L;
    for (int u = ulo + tid; u <= uhi; u += nt) {
      const int t = d - u;
      const int64_t n = base + (int64_t)t * U1 + u;
      const float ls = w.lse[n], lb = z[n * ld] - ls;
      float be = lb;
      if (t < len - 1 || u < L) {
        const float down = t < len - 1 ? buf[p][u] + lb : -INFINITY;
        const float right = u < L ? buf[p][u + 1] + (z[n * ld + lab[u]] - ls) : -INFINITY;
        be = logaddexp2f(down, right);
      }
      buf[p ^ 1][u] = be;
      w.beta[n] = be;
    }
    __syncthreads();
    p ^= 1;
  }
}

// dz[b][t][u][k] = g_b (softmax_k gamma - [k = 0] exp(alpha + lp_0 + beta(t+1, u) - log P)
//                                       - [k = y_{u+1}] exp(alpha + lp_k + beta(t, u+1) - log P)),  gamma = exp(alpha + beta - log P),
// beta(T_b, U_b) = 0 for the closing blank; zeros on padding and for an utterance that was not scored
__global__ __launch_bounds__(256) void rnnt_grad_kernel(int64_t nodes, int T, int U1, int V, const float* __restrict__ z,
                                                        int64_t ld, const int32_t* __restrict__ lens,
                                                        const int64_t* __restrict__ labels,
                                                        const int32_t* __restrict__ offs, const float* __restrict__ g,
                                                        RnntWs w, float* __restrict__ dz, int64_t lddz) {
  const int lane = threadIdx.x & 63;
  const int64_t node = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (node >= nodes) return;
  int b, t, u;
  node_of(node, T, U1, b, t, u);
  float* dzr = dz + node * lddz;
  const int len = clamp_len(lens[b], T), o0 = offs[b], L = clamp_labels(offs[b + 1] - o0, U1 - 1);
  const float lp = w.logp[b];
  if (t >= len || u > L || !(lp > -INFINITY)) {
    for (int k = lane; k < V; k += 64) dzr[k] = 0.f;
    return;
  }
  const float* zr = z + node * ld;
  const float a = w.alpha[node], be = w.beta[node], ls = w.lse[node], gb = g[b];
  const float gamma = expf((a + be) - lp);
  float cb = 0.f, cy = 0.f;
  if (t < len - 1) cb = expf(((a + (zr[0] - ls)) + w.beta[node + U1]) - lp);
  else if (u == L) cb = expf((a + (zr[0] - ls)) - lp);
  int yk = -1;
  if (u < L) {
    const int64_t v = labels[o0 + u];
    yk = (v < 1 || v >= V) ? 1 : (int)v;         // (an utterance with such a label was not scored: not reached)
    cy = expf(((a + (zr[yk] - ls)) + w.beta[node + 1]) - lp);
  }
  for (int k = lane; k < V; k += 64) {
    float d = expf(zr[k] - ls) * gamma;
    if (k == 0) d -= cb;
    if (k == yk) d -= cy;
    dzr[k] = gb * d;
  }
}

__global__ __launch_bounds__(256) void rnnt_greedy_step_kernel(int T, int J, int V, int L, int max_symbols,
                                                               const float* __restrict__ pe, const float* __restrict__ pp,
                                                               const float* __restrict__ w_out,
                                                               const float* __restrict__ b_out,
                                                               const int32_t* __restrict__ lens, int32_t* t_cur,
                                                               int32_t* n_out, int32_t* n_frame, int32_t* out, int32_t* last,
                                                               float* score, int32_t* advance) {
  extern __shared__ float sm[];
  float* zj = sm;                                // [J]
  float* lg = sm + J;                            // [V]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int t = t_cur[b], n = n_out[b], nf = n_frame[b];
  const int len = clamp_len(lens[b], T);
  __syncthreads();                               // every thread holds the row's state before thread 0 moves it
  if (t < 0 || t >= len || n < 0 || n >= L) {    // the row is done
    if (tid == 0) advance[b] = 0;
    return;
  }
  if (nf >= max_symbols) {                       // max_symbols tokens at this frame: on to the next one
    if (tid == 0) {
      t_cur[b] = t + 1;
      n_frame[b] = 0;
      advance[b] = 0;
    }
    return;
  }
  const float* per = pe + ((int64_t)b * T + t) * J;
  const float* ppr = pp + (int64_t)b * J;
  for (int j = tid; j < J; j += blockDim.x) zj[j] = tanhf(per[j] + ppr[j]);
  __syncthreads();
  for (int k = wave; k < V; k += nw) {
    const float* wr = w_out + (int64_t)k * J;
    float s = 0.f;
    for (int j = lane; j < J; j += 64) s += zj[j] * wr[j];
    s = wave_sum(s);
    if (lane == 0) lg[k] = s + (b_out ? b_out[k] : 0.f);
  }
  __syncthreads();
  if (wave != 0) return;
  float bv = -INFINITY;
  int bi = INT_MAX;
  for (int k = lane; k < V; k += 64)
    if (better(lg[k], k, bv, bi)) {
      bv = lg[k];
      bi = k;
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (better(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  float se = 0.f;
  for (int k = lane; k < V; k += 64) se += expf(lg[k] - bv);
  se = wave_sum(se);
  if (lane == 0) {
    if (bi <= 0 || bi >= V) {                    // blank (or no finite logit at all): the next frame
      t_cur[b] = t + 1;
      n_frame[b] = 0;
      advance[b] = 0;
    } else {
      out[(int64_t)b * L + n] = bi;
      last[b] = bi;
      n_out[b] = n + 1;
      n_frame[b] = nf + 1;
      score[b] += -logf(se);                     // logit - lse with the maximum as the logit: bv - (bv + log se)
      advance[b] = 1;
    }
  }
}

int rnnt_loss_check(int B, int T, int U, int V, int64_t ld, const void* ws, int64_t ws_bytes) {
  const int rc = rnnt_shape_check(B, T, U, 4, V);
  if (rc == ASR_E_ARG || ld < V || !ws) return ASR_E_ARG;
  if (rc) return rc;
  if (ws_bytes < rnnt_ws(nullptr, B, T, U + 1).bytes) return ASR_E_ARG;
  return 0;
}

}  // namespace

extern "C" int asr_rnnt_ws_bytes(int B, int T, int U, int J, int V, int64_t* ws_bytes) {
  if (!ws_bytes) return ASR_E_ARG;
  const int rc = rnnt_shape_check(B, T, U, J, V);
  if (rc) return rc;
  *ws_bytes = rnnt_ws(nullptr, B, T, U + 1).bytes;
  return 0;
}

extern "C" int asr_rnnt_joint_fwd_f32(int B, int T, int U, int J, const float* pe, const float* pp,
                                      const int32_t* frame_lens, const int32_t* label_offsets, float* z,
                                      asr_stream_t stream) {
  if (!pe || !pp || !frame_lens || !label_offsets || !z) return ASR_E_ARG;
  const int rc = rnnt_shape_check(B, T, U, J, 2);
  if (rc) return rc;
  if (!asr_aligned16(pe) || !asr_aligned16(pp) || !asr_aligned16(z)) return ASR_E_ALIGN;
  const int64_t total = (int64_t)B * T * (U + 1) * (J / 4);
  hipLaunchKernelGGL(rnnt_joint_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, total, T,
                     U + 1, J / 4, (const float4*)pe, (const float4*)pp, frame_lens, label_offsets, (float4*)z);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_rnnt_joint_bwd_f32(int B, int T, int U, int J, const float* dz, const float* z, const int32_t* frame_lens,
                                      const int32_t* label_offsets, float* dpe, float* dpp, asr_stream_t stream) {
  if (!dz || !z || !frame_lens || !label_offsets || !dpe || !dpp) return ASR_E_ARG;
  const int rc = rnnt_shape_check(B, T, U, J, 2);
  if (rc) return rc;
  if (!asr_aligned16(dz) || !asr_aligned16(z) || !asr_aligned16(dpe) || !asr_aligned16(dpp)) return ASR_E_ALIGN;
  const int64_t total = ((int64_t)B * T + (int64_t)B * (U + 1)) * (J / 4);
  hipLaunchKernelGGL(rnnt_joint_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B, T,
                     U + 1, J / 4, (const float4*)dz, (const float4*)z, frame_lens, label_offsets, (float4*)dpe, (float4*)dpp);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_rnnt_loss_fwd_f32(int B, int T, int U, int V, const float* logits, int64_t ld, const int32_t* frame_lens,
                                     const int64_t* labels, const int32_t* label_offsets, float* nll, void* ws,
                                     int64_t ws_bytes, asr_stream_t stream) {
  if (!logits || !frame_lens || !labels || !label_offsets || !nll) return ASR_E_ARG;
  const int rc = rnnt_loss_check(B, T, U, V, ld, ws, ws_bytes);
  if (rc) return rc;
  const RnntWs w = rnnt_ws(ws, B, T, U + 1);
  const int64_t nodes = (int64_t)B * T * (U + 1);
  hipLaunchKernelGGL(rnnt_lse_kernel, dim3((unsigned)((nodes + 3) / 4)), dim3(256), 0, (hipStream_t)stream, nodes, T, U + 1, V,
                     logits, ld, frame_lens, label_offsets, w.lse);
  ASR_CHECK_LAUNCH();
  hipLaunchKernelGGL(rnnt_alpha_kernel, dim3(B), dim3(U + 1 <= 64 ? 64 : 256), 0, (hipStream_t)stream, T, U + 1, V, logits, ld,
                     frame_lens, labels, label_offsets, nll, w);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_rnnt_loss_bwd_f32(int B, int T, int U, int V, const float* logits, int64_t ld, const int32_t* frame_lens,
                                     const int64_t* labels, const int32_t* label_offsets, const float* grad_nll, void* ws,
                                     int64_t ws_bytes, float* dlogits, int64_t lddz, asr_stream_t stream) {
  if (!logits || !frame_lens || !labels || !label_offsets || !grad_nll || !dlogits || lddz < V) return ASR_E_ARG;
  const int rc = rnnt_loss_check(B, T, U, V, ld, ws, ws_bytes);
  if (rc) return rc;
  const RnntWs w = rnnt_ws(ws, B, T, U + 1);
  const int64_t nodes = (int64_t)B * T * (U + 1);
  hipLaunchKernelGGL(rnnt_beta_kernel, dim3(B), dim3(U + 1 <= 64 ? 64 : 256), 0, (hipStream_t)stream, T, U + 1, V, logits, ld,
                     frame_lens, labels, label_offsets, w);
  ASR_CHECK_LAUNCH();
  hipLaunchKernelGGL(rnnt_grad_kernel, dim3((unsigned)((nodes + 3) / 4)), dim3(256), 0, (hipStream_t)stream, nodes, T, U + 1, V,
                     logits, ld, frame_lens, labels, label_offsets, grad_nll, w, dlogits, lddz);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_rnnt_greedy_step_f32(int B, int T, int J, int V, int L, int max_symbols, const float* pe, const float* pp,
                                        const float* w_out, const float* b_out, const int32_t* frame_lens, int32_t* t_cur,
                                        int32_t* n_out, int32_t* n_frame, int32_t* out, int32_t* last, float* score,
                                        int32_t* advance, asr_stream_t stream) {
  if (B <= 0 || T <= 0 || J <= 0 || V <= 0 || L <= 0 || max_symbols <= 0 || !pe || !pp || !w_out || !frame_lens || !t_cur ||
      !n_out || !n_frame || !out || !last || !score || !advance)
    return ASR_E_ARG;
  if (V < 2 || (J & 3) || ((int64_t)J + V) * 4 > kGreedyLds) return ASR_E_SHAPE;
  hipLaunchKernelGGL(rnnt_greedy_step_kernel, dim3(B), dim3(256), (size_t)(J + V) * 4, (hipStream_t)stream, T, J, V, L,
                     max_symbols, pe, pp, w_out, b_out, frame_lens, t_cur, n_out, n_frame, out, last, score, advance);
  ASR_CHECK_LAUNCH();
  return 0;
}
