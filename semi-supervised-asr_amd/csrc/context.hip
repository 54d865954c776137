// context.hip — the bias of token rows under their context graphs (the tables and the transition are
// context.h's):
//   context_score_kernel   one thread per row walks its graph from the root: an fp32 sum of the deltas in token order, then
//                          final of the last state - the operations of a search with the context inside, so a hypothesis'
//                          ctx_score is this kernel's output to the bit.  No atomics, one launch: the same bits in every run.
#include <limits.h>
#include "context.h"

namespace {

constexpr int kThreads = 64;

__global__ __launch_bounds__(kThreads) void context_score_kernel(int N, int L, ctx::Context g, const int32_t* __restrict__ graph_of,
                                                                 const int32_t* __restrict__ ids, int64_t ld,
                                                                 const int32_t* __restrict__ lens, float* __restrict__ score,
                                                                 float* __restrict__ tok) {
  const int n = blockIdx.x * kThreads + threadIdx.x;
  if (n >= N) return;
  const int len = lens[n] > L ? L : lens[n];
  const int32_t* row = ids + (int64_t)n * ld;
  float* trow = tok ? tok + (int64_t)n * L : nullptr;
  float sum = len < 0 ? -INFINITY : 0.f;                     // an unused slot scores -inf
  int state = ctx::graph_root(g, graph_of, n), i = 0;
  const bool on = state >= 0;                                // (off: no biasing for this row - bias 0, no state)
  for (; i < len; ++i) {
    const int c = row[i];
    if (c < 1 || c >= g.V) {                                 // not a token: the row scores NaN, nothing is indexed
      sum = NAN;
      break;
    }
    float d = 0.f;
    if (on) {
      state = ctx::step(g, state, c, &d);
      sum = __fadd_rn(sum, d);
    }
    if (trow) trow[i] = d;
  }
  if (trow)
    for (; i < L; ++i) trow[i] = sum != sum && i < len ? NAN : 0.f;
  if (on && len >= 0 && sum == sum) sum = ctx::finish(g, state, sum);
  score[n] = sum;
}

}  // namespace

extern "C" int asr_context_score_f32(int N, int L, const asr_context_t* c, const int32_t* graph_of, const int32_t* ids, int64_t ld,
                                     const int32_t* lens, float* score, float* tok_score, asr_stream_t stream) {
  if (N <= 0 || L <= 0 || !graph_of || !ids || !lens || !score || ld < L) return ASR_E_ARG;
  const int rc = ctx::check_abi(c);
  if (rc) return rc;
  hipLaunchKernelGGL(context_score_kernel, dim3((N + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, N, L,
                     ctx::from_abi(*c), graph_of, ids, ld, lens, score, tok_score);
  ASR_CHECK_LAUNCH();
  return 0;
}
