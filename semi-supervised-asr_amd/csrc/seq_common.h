// seq_common.h — what the sequence kernels over a [rows][V] logit matrix share: ctc.hip, ctc_align.hip, ctc_beam.hip,
// ctc_prefix.hip, rnnt_beam.hip, beam.hip and mwer.hip.  The conventions that make two-pass decoding, joint search and MWER
// agree to the bit live here and nowhere else:
//   blank = 0; the extended labels of a transcript are l' = (0, l_1, 0, l_2, ..., l_L, 0), S = 2L + 1 states
//   x[t][v] = z[t][v] - lse[t], with lse[t] = mx + logf(se) of wave_row_max_sumexp - no [rows][V] log-prob tensor exists
//   frames behind an utterance (t >= clamp_len(len, T)) are never read
//   candidates rank by greater value first, lower flat index on ties (better)
//   two entries of a beam are the same token sequence when hash (prefix_hash), length and last token agree: the merge
//   identity of ctc_beam.hip and rnnt_beam.hip, whose merged masses join by logaddexp
//   a search with an LM inside ranks by (tot + alpha lm) + beta len (lm_rank)
// No floating-point atomics, every sum in an order fixed by the shapes: the same bits in every run.
#pragma once
#include <limits.h>
#include "common.h"

namespace {

constexpr int kMaxL = ASR_CTC_MAX_LABELS;    // labels of a transcript: what ctc_shape_check admits and the chains size LDS for
constexpr int kMaxS = 2 * kMaxL + 1;
constexpr int kLseWaves = 4;                 // frames (waves) per workgroup of frame_lse_kernel

inline int64_t round64(int64_t n) { return (n + 63) / 64 * 64; }

__device__ __forceinline__ int clamp_len(int len, int T) { return len < 0 ? 0 : (len > T ? T : len); }

// candidate order: greater value first, lower flat index on ties
__device__ __forceinline__ bool better(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

typedef unsigned long long u64;

// log(exp a + exp b), symmetric in its arguments; (-inf) (+) (-inf) = -inf, and -inf (+) x = x exactly
// (not ctc_prefix.hip's lae: log1pf here, logf(1 + .) there - they round differently, and each search's bits are its own)
__device__ __forceinline__ float logaddexp(float a, float b) {
  const float m = fmaxf(a, b), n = fminf(a, b);
  if (n == -INFINITY) return m;
  return m + log1pf(expf(n - m));
}

// the hash of prefix . c from the hash of prefix (the splitmix64 finaliser over hash + token): with the length and the last
// token it stands for the token sequence (a collision of two different sequences of one length inside one beam would merge
// them: the odds, 2^-64 per pair, are accepted)
__device__ __forceinline__ u64 prefix_hash(u64 h, int c) {
  h += (u64)(unsigned)c + 0x9E3779B97F4A7C15ull;
  h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
  h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
  return h ^ (h >> 31);
}

// what a candidate of a search with an LM inside is ranked by: (tot + alpha lm) + beta len, fp32, every operation rounded on
// its own (no contraction into an fma) - tests/ngram_ref.py restates exactly this.  alpha = beta = 0 with a finite lm gives
// tot itself, so a plain search is the fused one at zero weights.
__device__ __forceinline__ float lm_rank(float tot, float lm, int len, float alpha, float beta) {
  return __fadd_rn(__fadd_rn(tot, __fmul_rn(alpha, lm)), __fmul_rn(beta, (float)len));
}

// One wave's pass over a row of V logits: lanes strided over V in ascending order, then the xor butterfly - the maximum,
// and the sum of exp(x - max).  Every lane ends with both; log-sum-exp = mx + logf(se).
__device__ __forceinline__ void wave_row_max_sumexp(const float* zr, int V, int lane, float& mx, float& se) {
  mx = -INFINITY;
  for (int v = lane; v < V; v += 64) mx = fmaxf(mx, zr[v]);
  mx = wave_max(mx);
  se = 0.f;
  for (int v = lane; v < V; v += 64) se += expf(zr[v] - mx);
  se = wave_sum(se);
}

// one wave per valid frame (b, t < len_b), WAVES frames per workgroup: lse[b][t] = logsumexp_v z[b][t][v]
// (a template, like its launcher: only the files that launch it carry it)
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void frame_lse_kernel(int B, int T, int V, const float* __restrict__ z, int64_t ld,
                                                               const int32_t* __restrict__ lens, float* __restrict__ lse) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (row >= (int64_t)B * T) return;
  const int b = (int)(row / T), t = (int)(row % T);
  if (t >= lens[b]) return;                                 // frames behind the utterance are never read
  float mx, se;
  wave_row_max_sumexp(z + row * ld, V, lane, mx, se);
  if (lane == 0) lse[row] = mx + logf(se);
}

// (the workgroups must fit a grid: ctc_shape_check's bound, for the default WAVES)
template <int WAVES = kLseWaves>
inline void launch_frame_lse(int B, int T, int V, const float* z, int64_t ld, const int32_t* lens, float* lse,
                             hipStream_t stream) {
  const unsigned groups = (unsigned)(((int64_t)B * T + WAVES - 1) / WAVES);
  hipLaunchKernelGGL(frame_lse_kernel<WAVES>, dim3(groups), dim3(64 * WAVES), 0, stream, B, T, V, z, ld, lens, lse);
}

// the sizes a CTC chain (loss, alignment) covers
inline int ctc_shape_check(int B, int T, int V, int Lmax) {
  if (B <= 0 || T <= 0 || V <= 0 || Lmax < 0) return ASR_E_ARG;
  if (V < 2 || Lmax > kMaxL || ((int64_t)B * T + kLseWaves - 1) / kLseWaves > 0x7fffffffLL) return ASR_E_SHAPE;
  return 0;
}

// A chain kernel by the states of its longest utterance, one workgroup per utterance: one wave up to 64 states, a state per
// thread up to 256, eight states per thread (strided over the workgroup) beyond.
template <typename K1, typename K8, typename... Args>
inline void launch_by_states(int Sp, K1 one, K8 eight, int B, hipStream_t stream, Args... args) {
  if (Sp <= 256) hipLaunchKernelGGL(one, dim3(B), dim3(Sp <= 64 ? 64 : 256), 0, stream, args...);
  else hipLaunchKernelGGL(eight, dim3(B), dim3(256), 0, stream, args...);
}

// The L labels of an utterance (labels[o0 ..]) into LDS.  -> false (for every thread) when the utterance cannot be scored:
// a label outside [1, V) or more labels than the launch was sized for.  Two barriers, which also order the caller's LDS
// fills before them.
__device__ __forceinline__ bool ctc_load_labels(const int64_t* __restrict__ labels, int o0, int L, int Lmax, int V, int* lab,
                                                int* bad) {
  if (threadIdx.x == 0) *bad = (L < 0 || L > Lmax) ? 1 : 0;
  __syncthreads();
  if (*bad) return false;
  for (int i = threadIdx.x; i < L; i += blockDim.x) {
    const int64_t v = labels[o0 + i];
    if (v < 1 || v >= V) atomicOr(bad, 1);
    lab[i] = (v < 1 || v >= V) ? 1 : (int)v;
  }
  __syncthreads();
  return *bad == 0;
}

// A thread's best M candidates (value v, flat index i), sorted by `better`, in two register arrays of the kernel (fully
// unrolled: no scratch), and plain functions over them.
template <int M>
__device__ __forceinline__ void top_clear(float (&v)[M], int (&i)[M]) {
#pragma unroll
  for (int j = 0; j < M; ++j) {
    v[j] = -INFINITY;
    i[j] = INT_MAX;
  }
}
// -inf and NaN never enter; a thread visits flat indices in ascending order, so an equal value never displaces an entry
template <int M>
__device__ __forceinline__ void top_insert(float (&v)[M], int (&i)[M], float c, int ci) {
  if (!(c > v[M - 1])) return;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const bool sw = better(c, ci, v[j], i[j]);
    const float tv = v[j];
    const int ti = i[j];
    v[j] = sw ? c : tv;
    i[j] = sw ? ci : ti;
    c = sw ? tv : c;
    ci = sw ? ti : ci;
  }
}
// the owner of a round's winner drops it
template <int M>
__device__ __forceinline__ void top_pop_if_head(float (&v)[M], int (&i)[M], int idx) {
  if (i[0] == idx) {
#pragma unroll
    for (int j = 0; j < M - 1; ++j) {
      v[j] = v[j + 1];
      i[j] = i[j + 1];
    }
    v[M - 1] = -INFINITY;
    i[M - 1] = INT_MAX;
  }
}

// One round of the workgroup arg-best over the threads' list heads (v, i) -> (bv, bi), the same in every thread; bv = -inf: no candidate
// is left.  EVERY thread of the workgroup calls it, the same number of times (it holds a barrier); nw waves (uniform);
// beyond one wave the wave winners meet in red_v / red_i [nw] behind ONE barrier, so the caller
// alternates between two pairs of buffers from round to round.
__device__ __forceinline__ void top_round(float v, int i, float* red_v, int* red_i, int nw, float& bv, int& bi) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off, 64);
    const int oi = __shfl_xor(i, off, 64);
    if (better(ov, oi, v, i)) {
      v = ov;
      i = oi;
    }
  }
  if (nw > 1) {
    if (lane == 0) {
      red_v[wave] = v;
      red_i[wave] = i;
    }
    __syncthreads();
    v = red_v[0];
    i = red_i[0];
    for (int w = 1; w < nw; ++w)
      if (better(red_v[w], red_i[w], v, i)) {
        v = red_v[w];
        i = red_i[w];
      }
  }
  bv = v;
  bi = i;
}

}  // namespace
