// word_lm.h — the device form of a word-level backoff n-gram LM behind a lexicon (the tables are word_lm.py's
// WordTable, validated by WordLM.compile(): the kernels trust every index).  Shared by word_lm.hip, ctc_beam.hip and rnnt_beam.hip.
//   the lexicon   a trie over token ids: trie_next int32 [N][V] (child node or -1; node 0 is the root), trie_word int32 [N]
//                 (the word id that ends at the node, or -1)
//   the LM        sparse: the arcs of state s are arc_off[s] .. arc_off[s + 1] - 1, arc_word ascending inside a state, with
//                 arc_logp and arc_next beside it; bo_logp / bo_state per state; the empty context is direct-indexed by the
//                 word: uni_logp / uni_next [W] (uni_next < 0: the word has no unigram and scores uni_logp = oov_logp from
//                 every context, the state going to the empty context)
// The lookup is one thread's: a binary search per level of the backoff chain, fp32, every addition rounded on its own.
#pragma once
#include <stdint.h>
#include "common.h"

namespace wlm {

struct WordLm {
  const int32_t* trie_next;
  const int32_t* trie_word;
  const int32_t* arc_off;
  const int32_t* arc_word;
  const float* arc_logp;
  const int32_t* arc_next;
  const float* bo_logp;
  const int32_t* bo_state;
  const float* uni_logp;
  const int32_t* uni_next;
  int V, space, start, empty, eos, unk;
};

inline WordLm from_abi(const asr_word_lm_t& t) {
  WordLm g;
  g.trie_next = t.trie_next, g.trie_word = t.trie_word, g.arc_off = t.arc_off, g.arc_word = t.arc_word;
  g.arc_logp = t.arc_logp, g.arc_next = t.arc_next, g.bo_logp = t.bo_logp, g.bo_state = t.bo_state;
  g.uni_logp = t.uni_logp, g.uni_next = t.uni_next;
  g.V = t.V, g.space = t.space, g.start = t.start, g.empty = t.empty, g.eos = t.eos, g.unk = t.unk;
  return g;
}

// 0 when the sizes and pointers of t can be walked at all (the CONTENTS are compile()'s to check)
inline int check_abi(const asr_word_lm_t* t) {
  if (!t || !t->trie_next || !t->trie_word || !t->arc_off || !t->arc_word || !t->arc_logp || !t->arc_next || !t->bo_logp ||
      !t->bo_state || !t->uni_logp || !t->uni_next || t->V <= 0 || t->N <= 0 || t->S <= 0 || t->W <= 0 || t->A < 0)
    return ASR_E_ARG;
  if (t->V < 2 || (int64_t)t->N * t->V > 0x7fffffffLL || t->space < 1 || t->space >= t->V || t->start < 0 || t->start >= t->S ||
      t->empty < 0 || t->empty >= t->S || t->eos < 0 || t->eos >= t->W || t->unk < 0 || t->unk >= t->W)
    return ASR_E_SHAPE;
  return 0;
}

// (state s, word w) -> (lp, next): down the backoff chain of s until an arc of w is listed, the empty context at its bottom
__device__ __forceinline__ void lookup(const WordLm& g, int s, int w, float& lp, int& next) {
  const int un = g.uni_next[w];
  const float ul = g.uni_logp[w];
  if (un < 0) {                                              // no unigram: oov_logp whatever the context
    lp = ul;
    next = g.empty;
    return;
  }
  float acc = 0.f;
  while (s != g.empty) {
    int lo = g.arc_off[s];
    const int end = g.arc_off[s + 1];
    int hi = end;
    while (lo < hi) {                                        // the first arc whose word is not below w
      const int mid = lo + ((hi - lo) >> 1);
      if (g.arc_word[mid] < w) lo = mid + 1;
      else hi = mid;
    }
    if (lo < end && g.arc_word[lo] == w) {
      lp = __fadd_rn(acc, g.arc_logp[lo]);
      next = g.arc_next[lo];
      return;
    }
    acc = __fadd_rn(acc, g.bo_logp[s]);
    s = g.bo_state[s];
  }
  lp = __fadd_rn(acc, ul);
  next = un;
}

// the word that is pending at trie node `node` (!= the root; < 0: the tokens left the trie) closes from word state s.  A
// node that ends no word is <unk> - or, with lexicon_only, no word at all: next = -1 and lp = 0.
__device__ __forceinline__ void close_word(const WordLm& g, int node, int s, bool lexicon_only, float& lp, int& next) {
  int w = node < 0 ? -1 : g.trie_word[node];
  if (w < 0) {
    if (lexicon_only) {
      lp = 0.f;
      next = -1;
      return;
    }
    w = g.unk;
  }
  lookup(g, s, w, lp, next);
}

// the trie node after token c (c in 0 .. V-1) from `node` (< 0: off the trie, and it stays there)
__device__ __forceinline__ int trie_step(const WordLm& g, int node, int c) {
  return node < 0 ? -1 : g.trie_next[(int64_t)node * g.V + c];
}

// The word position of a hypothesis - a function of its token sequence - and its transitions, one thread's.  The searches
// (ctc_beam.hip, rnnt_beam.hip) move through these and nothing else; the scorer (word_lm.hip) spells the same walk out for a
// row, and a search's lm_score must be the scorer's to the bit: lm is the fp32 sum over the COMPLETED words in word order, every addition
// rounded on its own; as a complete hypothesis the pending word joins first, then the end-of-sentence term.
struct WordPos {
  int node, state;         // the trie node of the pending word (0: the root, none pending; < 0: off the trie), the word state
  float lm;
  int nw;                  // the completed words
};

__device__ __forceinline__ WordPos start_pos(const WordLm& g) { return WordPos{0, g.start, 0.f, 0}; }

// the close pair of the pending word: what a <space> and the end of the hypothesis add, and the state behind it
// ((0, state) at the root; next < 0: lexicon_only and the node ends no word).  A search looks it up once per entry.
__device__ __forceinline__ void close_pair(const WordLm& g, int node, int state, bool lexicon_only, float& lp, int& next) {
  lp = 0.f;
  next = state;
  if (node != 0) close_word(g, node, state, lexicon_only, lp, next);
}

// the position after the non-blank token c, (lp, next) being p's close pair: only a <space> behind a pending word closes it
__device__ __forceinline__ WordPos after_token(const WordLm& g, WordPos p, int c, float lp, int next) {
  if (c != g.space) {
    p.node = trie_step(g, p.node, c);
  } else if (p.node != 0) {
    p.lm = __fadd_rn(p.lm, lp);
    p.nw += 1;
    p.state = next;
    p.node = 0;
  }
  return p;
}

// p as a complete hypothesis, (lp, next) being its close pair.  -> false: no hypothesis (lexicon_only and the pending node
// ends no word)
__device__ __forceinline__ bool finish(const WordLm& g, WordPos& p, float lp, int next, bool eos_term) {
  if (p.node != 0) {
    if (next < 0) return false;
    p = after_token(g, p, g.space, lp, next);
  }
  if (eos_term) {
    float el;
    int en;
    lookup(g, p.state, g.eos, el, en);
    p.lm = __fadd_rn(p.lm, el);
  }
  return true;
}

}  // namespace wlm
