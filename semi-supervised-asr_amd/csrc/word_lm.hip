// word_lm.hip — scoring token rows with a word-level backoff n-gram LM behind a lexicon (the tables and the
// lookup are word_lm.h's).
//   word_lm_score_kernel   one thread per row: the tokens walk the trie, a <space> behind a pending word closes it (one
//                          lookup from the row's word state), the fp32 sum runs in word order, then the pending word and
//                          the end-of-sentence term.  No atomics, one launch: the same bits in every run.
#include <limits.h>
#include "word_lm.h"

namespace {

constexpr int kThreads = 64;

__global__ __launch_bounds__(kThreads) void word_lm_score_kernel(int N, int L, wlm::WordLm g, int eos_term,
                                                                 const int32_t* __restrict__ ids, int64_t ld,
                                                                 const int32_t* __restrict__ lens, float* __restrict__ score,
                                                                 int32_t* __restrict__ n_words, float* __restrict__ word_score) {
  const int n = blockIdx.x * kThreads + threadIdx.x;
  if (n >= N) return;
  const int len = lens[n] > L ? L : lens[n];
  const int32_t* row = ids + (int64_t)n * ld;
  float* wrow = word_score ? word_score + (int64_t)n * L : nullptr;
  float sum = len < 0 ? -INFINITY : 0.f;                     // an unused slot scores -inf
  int state = g.start, node = 0, nw = 0;
  bool bad = false;
  for (int i = 0; i < len; ++i) {
    const int c = row[i];
    if (c < 0 || c >= g.V) {                                 // not a token: the row scores NaN, nothing is indexed
      bad = true;
      break;
    }
    if (c != g.space) {
      node = wlm::trie_step(g, node, c);
    } else if (node != 0) {
      float lp;
      int nx;
      wlm::close_word(g, node, state, false, lp, nx);
      sum += lp;
      if (wrow) wrow[nw] = lp;
      ++nw;
      state = nx;
      node = 0;
    }
  }
  if (!bad && len >= 0) {
    if (node != 0) {
      float lp;
      int nx;
      wlm::close_word(g, node, state, false, lp, nx);
      sum += lp;
      if (wrow) wrow[nw] = lp;
      ++nw;
      state = nx;
    }
    if (eos_term) {
      float lp;
      int nx;
      wlm::lookup(g, state, g.eos, lp, nx);
      sum += lp;
    }
  }
  if (wrow)
    for (int j = nw; j < L; ++j) wrow[j] = 0.f;              // (a row of L tokens holds at most (L + 1) / 2 <= L words)
  score[n] = bad ? NAN : sum;
  n_words[n] = nw;
}

}  // namespace

extern "C" int asr_word_lm_score_f32(int N, int L, const asr_word_lm_t* lm, int eos_term, const int32_t* ids, int64_t ld,
                                     const int32_t* lens, float* score, int32_t* n_words, float* word_score,
                                     asr_stream_t stream) {
  if (N <= 0 || L <= 0 || !ids || !lens || !score || !n_words || ld < L) return ASR_E_ARG;
  const int rc = wlm::check_abi(lm);
  if (rc) return rc;
  hipLaunchKernelGGL(word_lm_score_kernel, dim3((N + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, N, L,
                     wlm::from_abi(*lm), eos_term, ids, ld, lens, score, n_words, word_score);
  ASR_CHECK_LAUNCH();
  return 0;
}
