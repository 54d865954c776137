// context.h — the device form of the context graphs of contextual biasing (the tables are context.py's
// ContextTable, validated where they are compiled: the kernels trust every index).  Shared by context.hip and ctc_beam.hip, so
// that the scorer and the search execute the same operations.
//   a state s     its transitions that differ from its default row are the arcs arc_off[s] .. arc_off[s + 1] - 1, arc_tok
//                 ascending inside a state with arc_next beside it; every other token goes where the default row says:
//                 dflt[drow[s]][c].  The failure links are resolved on the host: no loop over them here.
//   credit, pending fp32 [N]   delta(s, c) = credit[next(s, c)] - pending[s], one fp32 subtraction; a hypothesis that ends in
//                 s gives pending[s] back (finish)
//   root int32 [G]             the root of graph g; the states of all graphs share one numbering
// A transition is one thread's: a binary search over the state's arcs, then at most one read of the default row.
#pragma once
#include <stdint.h>
#include "common.h"

namespace ctx {

struct Context {
  const int32_t* arc_off;
  const int32_t* arc_tok;
  const int32_t* arc_next;
  const int32_t* drow;
  const int32_t* dflt;
  const float* credit;
  const float* pending;
  const int32_t* root;
  int V, G;
};

inline Context from_abi(const asr_context_t& t) {
  Context g;
  g.arc_off = t.arc_off, g.arc_tok = t.arc_tok, g.arc_next = t.arc_next, g.drow = t.drow, g.dflt = t.dflt;
  g.credit = t.credit, g.pending = t.pending, g.root = t.root;
  g.V = t.V, g.G = t.G;
  return g;
}

// 0 when the sizes and pointers of t can be walked at all (the CONTENTS are the host compiler's to check)
inline int check_abi(const asr_context_t* t) {
  if (!t || !t->arc_off || !t->arc_tok || !t->arc_next || !t->drow || !t->dflt || !t->credit || !t->pending || !t->root)
    return ASR_E_ARG;
  if (t->V < 2 || t->N <= 0 || t->G <= 0 || t->G > t->N || t->R < t->G || t->R > t->N || t->A < 0 || t->A > 0x7fffffffLL ||
      (int64_t)t->R * t->V > 0x7fffffffLL)
    return ASR_E_SHAPE;
  return 0;
}

// what the transitions of state s share: its arcs, its default row and what it has been lent
struct Node {
  int lo, hi;
  const int32_t* row;
  float pending;
};

__device__ __forceinline__ Node node(const Context& g, int s) {
  return Node{g.arc_off[s], g.arc_off[s + 1], g.dflt + (int64_t)g.drow[s] * g.V, g.pending[s]};
}

// the state after token c (1 .. V-1) from the state n was read for, and the transition's delta
__device__ __forceinline__ int arc(const Context& g, const Node& n, int c, float* delta) {
  int lo = n.lo, hi = n.hi;
  while (lo < hi) {                                          // the first arc whose token is not below c
    const int mid = lo + ((hi - lo) >> 1);
    if (g.arc_tok[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  const int next = lo < n.hi && g.arc_tok[lo] == c ? g.arc_next[lo] : n.row[c];
  *delta = __fsub_rn(g.credit[next], n.pending);
  return next;
}

__device__ __forceinline__ int step(const Context& g, int state, int c, float* delta) { return arc(g, node(g, state), c, delta); }

// bias as that of a complete hypothesis that ends in `state`: final(state) = -pending[state] joins it
__device__ __forceinline__ float finish(const Context& g, int state, float bias) { return __fsub_rn(bias, g.pending[state]); }

// the graph of a row: graph_of[row] in 0 .. G-1, anything else (-1) is no biasing
__device__ __forceinline__ int graph_root(const Context& g, const int32_t* graph_of, int64_t row) {
  const int gi = graph_of[row];
  return gi >= 0 && gi < g.G ? g.root[gi] : -1;
}

}  // namespace ctx
