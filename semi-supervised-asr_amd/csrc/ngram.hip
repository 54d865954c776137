// ngram.hip — scoring label sequences with a compiled backoff n-gram LM (the table is ngram.py's NgramTable):
//   logp fp32 [S][V]   ln p(c | state) with the backoffs resolved on the host;   next int32 [S][V]   the state after c
// The table is trusted: NgramLM.compile() has checked 0 <= next < S and S V < 2^31.
//   ngram_score_kernel   one thread per sequence walks the automaton from `start`: an fp32 sum in token order, then the
//                        end-of-sentence term.  No atomics, one launch: the same bits in every run.
#include <limits.h>
#include "common.h"

namespace {

constexpr int kThreads = 64;

__global__ __launch_bounds__(kThreads) void ngram_score_kernel(int N, int L, int V, const float* __restrict__ logp,
                                                               const int32_t* __restrict__ next, int start, int eos,
                                                               const int32_t* __restrict__ ids, int64_t ld,
                                                               const int32_t* __restrict__ lens, float* __restrict__ score,
                                                               float* __restrict__ tok) {
  const int n = blockIdx.x * kThreads + threadIdx.x;
  if (n >= N) return;
  const int len = lens[n] > L ? L : lens[n];
  const int32_t* row = ids + (int64_t)n * ld;
  float* trow = tok ? tok + (int64_t)n * L : nullptr;
  float sum = len < 0 ? -INFINITY : 0.f;                     // an unused slot scores -inf
  int state = start, i = 0;
  for (; i < len; ++i) {
    const int c = row[i];
    if (c < 0 || c >= V) {                                   // not a token: the sequence scores NaN, nothing is indexed
      sum = NAN;
      break;
    }
    const int64_t at = (int64_t)state * V + c;
    const float lp = logp[at];
    sum += lp;
    if (trow) trow[i] = lp;
    state = next[at];
  }
  if (trow)
    for (; i < L; ++i) trow[i] = sum != sum && i < len ? NAN : 0.f;
  if (eos >= 0 && len >= 0) sum += logp[(int64_t)state * V + eos];        // (NaN stays NaN; state is still a state)
  score[n] = sum;
}

}  // namespace

extern "C" int asr_ngram_score_f32(int N, int L, int S, int V, const float* logp, const int32_t* next, int start, int eos,
                                   const int32_t* ids, int64_t ld, const int32_t* lens, float* score, float* tok_score,
                                   asr_stream_t stream) {
  if (N <= 0 || L <= 0 || S <= 0 || V <= 0 || !logp || !next || !ids || !lens || !score || ld < L) return ASR_E_ARG;
  if (V < 2 || (int64_t)S * V > INT_MAX || start < 0 || start >= S || eos >= V) return ASR_E_SHAPE;
  hipLaunchKernelGGL(ngram_score_kernel, dim3((N + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, N, L, V,
                     logp, next, start, eos, ids, ld, lens, score, tok_score);
  ASR_CHECK_LAUNCH();
  return 0;
}
