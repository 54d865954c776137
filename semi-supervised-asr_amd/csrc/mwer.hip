// mwer.hip — minimum (word) error rate training on an n-best list: the expected number of edit errors under the model's
// sequence probabilities renormalised over the list (Prabhavalkar et al. 2018), forward and backward.
// Rows are r = b K + k (utterance b, hypothesis k), R = B K.  logits [L][R][V] fp32 time-major (row stride ld), tokens int64
// [L][R] (the hypothesis with its <EOS>, <EOS>-padded), npos int32 [R] (n_r = the scored positions, clamped to 1 .. L;
// <= 0: an unused slot), err int32 [R] (the edit distance to the utterance's reference), scale (the caller's 1 / B).
//   s_r     = sum_{l < n_r} (logits[l][r][tokens[l][r]] - logsumexp_v logits[l][r][:])            in increasing l
//   over the live slots of utterance b, with m_b = max_k s_k and Wbar_b = the mean of err:
//   phat_r  = exp(s_r - m_b) / sum_j exp(s_j - m_b)                                              the sum in increasing j
//   risk_b  = sum_k phat_k (err_k - Wbar_b)                                                      in increasing k
//   coef_r  = phat_r (err_r - Wbar_b - risk_b)                                                   = d risk_b / d s_r
//   loss    = scale sum_b risk_b                                                                 in increasing b
//   an unused slot has s = phat = coef = 0; an utterance without a live slot has risk = 0
//   dlogits[l][r][v] = g scale coef_r (1[v = tokens[l][r]] - softmax(logits[l][r][:])_v)  for l < n_r;  exact zeros for
//                      l >= n_r and for unused rows, whose logits are not read (nor are those of a row with coef_r = 0)
// Three kernels, no floating-point atomics, every sum in an order fixed by the shapes:
//   mwer_logp_kernel    one wave per (l, r) with l < n_r: the log-softmax of the row (seq_common.h's row pass)
//                       and the gather -> lp[l][r] in the workspace; positions behind n_r are neither read nor written
//   mwer_risk_kernel    ONE workgroup: a thread per row sums lp over l (rows strided over the threads: the loads of a step
//                       are coalesced and independent, only the adds chain), a thread per utterance then walks its K <= 16
//                       slots three times (maximum and error mean; normaliser; risk) and writes phat, coef and risk, and
//                       thread 0 adds the B risks.  Nothing is reduced across threads, so no order depends on scheduling.
//   mwer_grad_kernel    one wave per (l, r): the row's softmax again (V is small) and the scaled difference, or zeros
#include "seq_common.h"

namespace {

constexpr int kMaxK = ASR_BEAM_KMAX;

__device__ __forceinline__ int mwer_npos(const int32_t* __restrict__ npos, int r, int L) {
  return clamp_len(npos[r], L);
}

// a token outside [0, V) is read as the nearest valid one: no access leaves the row
__device__ __forceinline__ int mwer_token(const int64_t* __restrict__ tokens, int64_t row, int V) {
  const int64_t t = tokens[row];
  return t < 0 ? 0 : (t >= V ? V - 1 : (int)t);
}

__global__ __launch_bounds__(256) void mwer_logp_kernel(int R, int L, int V, const float* __restrict__ z, int64_t ld,
                                                        const int64_t* __restrict__ tokens,
                                                        const int32_t* __restrict__ npos, float* __restrict__ lp) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (int64_t)L * R) return;
  const int l = (int)(row / R), r = (int)(row % R);
  if (l >= mwer_npos(npos, r, L)) return;
  const float* zr = z + row * ld;
  float mx, se;
  wave_row_max_sumexp(zr, V, lane, mx, se);
  if (lane == 0) lp[row] = zr[mwer_token(tokens, row, V)] - (mx + logf(se));
}

__global__ __launch_bounds__(256) void mwer_risk_kernel(int B, int K, int L, const float* __restrict__ lp,
                                                        const int32_t* __restrict__ npos, const int32_t* __restrict__ err,
                                                        float scale, float* __restrict__ seq_logp, float* __restrict__ post,
                                                        float* __restrict__ coef, float* __restrict__ risk,
                                                        float* __restrict__ loss) {
  const int R = B * K, tid = threadIdx.x, nt = blockDim.x;
  for (int r = tid; r < R; r += nt) {
    const int n = mwer_npos(npos, r, L);
    float s = 0.f;
    for (int l = 0; l < n; ++l) s += lp[(int64_t)l * R + r];
    seq_logp[r] = s;
  }
  __syncthreads();                                          // (workgroup scope: the sums above are visible below)
  for (int b = tid; b < B; b += nt) {
    const int r0 = b * K;
    float m = -INFINITY;
    int live = 0, esum = 0;
    for (int k = 0; k < K; ++k)
      if (npos[r0 + k] > 0) {
        m = fmaxf(m, seq_logp[r0 + k]);
        esum += err[r0 + k];
        ++live;
      }
    float rb = 0.f;
    if (live == 0) {
      for (int k = 0; k < K; ++k) post[r0 + k] = coef[r0 + k] = 0.f;
    } else {
      const float wbar = (float)esum / (float)live;
      float zsum = 0.f;
      for (int k = 0; k < K; ++k)
        if (npos[r0 + k] > 0) zsum += expf(seq_logp[r0 + k] - m);
      const float inv = 1.0f / zsum;
      float p[kMaxK];
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) {
        p[k] = 0.f;
        if (k < K && npos[r0 + k] > 0) {
          p[k] = expf(seq_logp[r0 + k] - m) * inv;
          rb += p[k] * ((float)err[r0 + k] - wbar);
        }
      }
#pragma unroll
      for (int k = 0; k < kMaxK; ++k)
        if (k < K) {
          const bool on = npos[r0 + k] > 0;
          post[r0 + k] = p[k];
          coef[r0 + k] = on ? p[k] * (((float)err[r0 + k] - wbar) - rb) : 0.f;
        }
    }
    risk[b] = rb;
  }
  __syncthreads();
  if (tid == 0) {
    float tot = 0.f;
    for (int b = 0; b < B; ++b) tot += risk[b];
    loss[0] = scale * tot;
  }
}

__global__ __launch_bounds__(256) void mwer_grad_kernel(int R, int L, int V, const float* __restrict__ z, int64_t ld,
                                                        const int64_t* __restrict__ tokens,
                                                        const int32_t* __restrict__ npos, const float* __restrict__ coef,
                                                        const float* __restrict__ g, float gscale, float* __restrict__ dz,
                                                        int64_t lddz) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (int64_t)L * R) return;
  const int l = (int)(row / R), r = (int)(row % R);
  float* dzr = dz + row * lddz;
  const float c = coef[r];
  if (l >= mwer_npos(npos, r, L) || c == 0.f) {              // (wave-uniform) masked, unused, or no gradient at all
    for (int v = lane; v < V; v += 64) dzr[v] = 0.f;
    return;
  }
  const float* zr = z + row * ld;
  float mx, se;
  wave_row_max_sumexp(zr, V, lane, mx, se);
  const float inv = 1.0f / se, gr = g[0] * gscale * c;
  const int tok = mwer_token(tokens, row, V);
  for (int v = lane; v < V; v += 64) dzr[v] = gr * ((v == tok ? 1.f : 0.f) - expf(zr[v] - mx) * inv);
}

int mwer_check(int B, int K, int L, int V, int64_t ld) {
  if (B <= 0 || K <= 0 || L <= 0 || V <= 0 || ld < V) return ASR_E_ARG;
  if (K > kMaxK || (int64_t)B * K > 0x7fffffffLL || ((int64_t)B * K * L + 3) / 4 > 0x7fffffffLL) return ASR_E_SHAPE;
  return 0;
}

}  // namespace

extern "C" int asr_mwer_fwd_f32(int B, int K, int L, int V, const float* logits, int64_t ld, const int64_t* tokens,
                                const int32_t* npos, const int32_t* err, float scale, float* seq_logp, float* post,
                                float* coef, float* risk, float* loss, float* ws, int64_t ws_bytes, asr_stream_t stream) {
  if (!logits || !tokens || !npos || !err || !seq_logp || !post || !coef || !risk || !loss || !ws) return ASR_E_ARG;
  const int rc = mwer_check(B, K, L, V, ld);
  if (rc) return rc;
  const int R = B * K;
  if (ws_bytes < 4 * (int64_t)L * R) return ASR_E_ARG;
  const unsigned rows4 = (unsigned)(((int64_t)L * R + 3) / 4);
  hipLaunchKernelGGL(mwer_logp_kernel, dim3(rows4), dim3(256), 0, (hipStream_t)stream, R, L, V, logits, ld, tokens, npos, ws);
  ASR_CHECK_LAUNCH();
  hipLaunchKernelGGL(mwer_risk_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, B, K, L, ws, npos, err, scale, seq_logp,
                     post, coef, risk, loss);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_mwer_bwd_f32(int B, int K, int L, int V, const float* logits, int64_t ld, const int64_t* tokens,
                                const int32_t* npos, const float* coef, const float* grad_loss, float grad_scale,
                                float* dlogits, int64_t lddz, asr_stream_t stream) {
  if (!logits || !tokens || !npos || !coef || !grad_loss || !dlogits || lddz < V) return ASR_E_ARG;
  const int rc = mwer_check(B, K, L, V, ld);
  if (rc) return rc;
  const int R = B * K;
  const unsigned rows4 = (unsigned)(((int64_t)L * R + 3) / 4);
  hipLaunchKernelGGL(mwer_grad_kernel, dim3(rows4), dim3(256), 0, (hipStream_t)stream, R, L, V, logits, ld, tokens, npos,
                     coef, grad_loss, grad_scale, dlogits, lddz);
  ASR_CHECK_LAUNCH();
  return 0;
}
