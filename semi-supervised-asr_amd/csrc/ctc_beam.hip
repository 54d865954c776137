// ctc_beam.hip — CTC prefix beam search over the CTC head's logits: the n-best list of the head itself, the
// first pass of two-pass decoding.  The conventions are seq_common.h's; its frame_lse_kernel runs first.
//   ctc_beam_kernel       one workgroup per utterance (one wave when K V <= kOneWaveKV, four beyond), looping over its frames.
//                         The beam (at most K prefixes: pb, pnb, tot, last token, length, 64-bit prefix hash) lives in LDS, two
//                         slots.  Per frame:
//                           merge map  thread j < live: the beam entries that are prefix_j + one token (hash of the extension,
//                                      length + 1) as a bit mask - those extensions are not candidates
//                           candidates thread j < live forms the stay candidate of entry j (flat index j), the masses of the
//                                      extensions that ARE entry j added to its pnb' in ascending entry order; all threads walk
//                                      the extensions (entry-major, tokens strided over the threads: ascending flat index
//                                      K + k (V - 1) + (c - 1)) and keep their best M >= K in a sorted register list (top_insert)
//                           select     K rounds of a workgroup arg-best over the list heads (seq_common.h's order; -inf
//                                      never wins); the thread whose number is the round keeps the winner
//                           update     thread r < selected writes entry r of the other slot and (parent slot, token) of the
//                                      frame into the history - LDS when T_b K entries fit kHistLds, the workspace otherwise
//                         The emissions of the frame ahead are in registers (kStage tokens per thread) while a frame runs and go
//                         to LDS at its end; a token behind kStage * threads is read from memory where it is used.
//                         After the last frame the beam IS the ranking (the select's order): thread r walks the history of
//                         entry r back into hyp[r].  The same tail serves the word-LM mode, which finishes and ranks its
//                         entries first; the n-gram mode has its own.
//   ctc_beam_kernel<M, kNgram>   the search with an n-gram LM inside (the table is ngram.hip's): an entry also
//                         carries its automaton state and lm, the fp32 sum of logp[state][c] over its tokens in order - both
//                         functions of the token sequence, so equal prefixes hold equal bits and the merge is unchanged.  The
//                         masses pb / pnb / tot are the plain kernel's, operation for operation; only the value a candidate
//                         is ranked by differs (lm_rank).  The LM row of an entry is read through L2 where it is used: one
//                         coalesced read per (entry, token), beside the emission's.  The list holds ranks, so update forms
//                         the winner's mass again (the same operations on the same operands: the same bits).  After the last
//                         frame the end-of-sentence term joins lm and the (at most K) entries are ranked once more.
//   ctc_beam_kernel<M, kWordLm>   the search with a lexicon and a word-level n-gram LM inside (the tables and
//                         the lookup are word_lm.h's): an entry carries its trie node, its word state, lm (the fp32 sum over
//                         its COMPLETED words) and nw (their count) - again functions of the token sequence - and the "close"
//                         pair (lp, next state) of its pending word, looked up ONCE by the thread that creates the entry
//                         (update) and read from LDS by the candidate walk; a stay entry copies it.  Only an extension by
//                         <space> from a node that is not the root changes lm and nw (word_lm.h's after_token; the tail and
//                         an utterance without frames use its finish).  Ranks are lm_rank's with nw for len.
//                         With lexicon_only the walk also reads the entry's trie row (one coalesced read per (entry, token),
//                         as the n-gram variant reads its LM row) and drops what leaves the lexicon.
//   ctc_beam_kernel<M, kCtx>, <M, kNgramCtx>   the search with a context graph per utterance inside, alone or beside the
//                         n-gram LM (the tables and the transition are context.h's): an entry also carries its
//                         context state and bias, the fp32 sum of its deltas in token order - functions of the token
//                         sequence again.  The candidate walk takes the step per (entry, token) where the n-gram mode reads
//                         its LM row; a candidate ranks by what the search without a context would rank it by, plus
//                         ctx_weight bias as the last operation; update forms the winner's state again.  After the last
//                         frame final of the state joins bias and the entries rank once more (the n-gram mode's tail).  An
//                         utterance whose graph index is -1 never moves: its bias stays 0 and its ranks are the plain ones.
#include <float.h>
#include <type_traits>
#include "seq_common.h"
#include "context.h"
#include "word_lm.h"

namespace {

constexpr int kKmax = ASR_BEAM_KMAX;
constexpr int kStage = 4;                                  // emissions a thread holds a frame ahead
constexpr int kMaxThreads = 256;
constexpr int kOneWaveKV = ASR_CTC_BEAM_ONE_WAVE_KV;       // K V up to this: one wave per utterance
constexpr int kHistLds = ASR_CTC_BEAM_LDS_ENTRIES;         // (frame, slot) history entries that stay in LDS
static_assert(kKmax <= 32, "the merge map of an entry is one 32-bit mask");
// (2048: the beam's two slots, the candidates' and the reduction's arrays - at most, with the word LM inside: 17 words per
// entry, the state, lm and stay mass of a search with an LM 5, and node, nw and the close pair in two slots each 8; the
// n-gram mode's rank and position are 2 in their place, and a context's state and bias in two slots 4 more)
static_assert(kHistLds * 8 + kStage * kMaxThreads * 4 + 2048 <= 64 * 1024, "the static LDS of a workgroup");
static_assert((17 + 5 + 4 * 2) * 4 * kKmax + 2 * 2 * (kMaxThreads / 64) * 4 <= 2048,
              "the beam's arrays of the word-LM variant inside the 2048 bytes above");
static_assert((17 + 5 + 2 + 2 * 2) * 4 * kKmax + 2 * 2 * (kMaxThreads / 64) * 4 <= 2048,
              "the beam's arrays of the n-gram + context variant inside the 2048 bytes above");

struct BeamWs {
  int2* hist;      // [B][T][K] (parent slot, token; token 0: the entry stayed); absent when T K entries fit LDS
  float* lse;      // [B][T]
  int64_t bytes;
};

BeamWs beam_ws(void* base, int B, int T, int K) {
  const int64_t n_h = (int64_t)T * K > kHistLds ? (int64_t)B * T * K : 0;
  BeamWs w;
  w.hist = (int2*)base;                                      // (first: 8-byte aligned wherever the workspace is)
  w.lse = (float*)(w.hist + n_h);
  w.bytes = 8 * n_h + 4 * round64((int64_t)B * T);
  return w;
}

// the LM of a fused search (LM = true; all zero otherwise and never read)
struct BeamLm {
  const float* logp;       // [S][V]
  const int32_t* next;     // [S][V]
  float* ctc_score;        // [B][K]
  float* lm_score;         // [B][K]
  int start, eos;          // eos < 0: no end-of-sentence term
  float alpha, beta;
};

// the lexicon and word LM of a fused search (MODE = kWordLm)
struct BeamWlm {
  wlm::WordLm w;
  float* ctc_score;        // [B][K]
  float* lm_score;         // [B][K]
  int32_t* n_words;        // [B][K]
  float alpha, beta;
  int eos_term, lexicon_only;
};

// the context of a fused search beside its LM (MODE = kCtx: no LM, its part all zero but ctc_score; kNgramCtx)
struct BeamCtx : BeamLm {
  ctx::Context c;
  const int32_t* graph_of; // [B]
  float* ctx_score;        // [B][K]
  float weight;
};

constexpr int kPlain = 0, kNgram = 1, kWordLm = 2, kCtx = 3, kNgramCtx = 4;      // what sits inside the search

template <int MODE>
using BeamArg = std::conditional_t<MODE == kWordLm, BeamWlm, std::conditional_t<MODE == kCtx || MODE == kNgramCtx, BeamCtx, BeamLm>>;

// the rank of a search with a context inside: the rank without one, plus weight bias as the last operation
__device__ __forceinline__ float ctx_rank(float rank, float weight, float bias) { return __fadd_rn(rank, __fmul_rn(weight, bias)); }

template <int M, int MODE>
__global__ __launch_bounds__(kMaxThreads) void ctc_beam_kernel(int T, int V, int K, const float* __restrict__ z, int64_t ld,
                                                               const int32_t* __restrict__ lens, int32_t* __restrict__ hyp,
                                                               int32_t* __restrict__ hyp_len, float* __restrict__ score,
                                                               BeamWs w, BeamArg<MODE> g) {
  constexpr bool LM = MODE == kNgram || MODE == kNgramCtx, WLM = MODE == kWordLm, CX = MODE == kCtx || MODE == kNgramCtx;
  constexpr bool RK = MODE != kPlain;                        // RK: the list holds ranks
  __shared__ int s_cst[2][kKmax];                            // (context only: the state and the bias of an entry)
  __shared__ float s_bias[2][kKmax];
  __shared__ int s_state[2][kKmax], s_pos[kKmax];            // (LM only, like the next line: unused arrays take no LDS)
  __shared__ float s_lm[2][kKmax], s_stot[kKmax], s_rank[kKmax];
  __shared__ int s_node[2][kKmax], s_nw[2][kKmax], s_cnx[2][kKmax];      // (word LM only: trie node, words, close pair)
  __shared__ float s_clp[2][kKmax];
  __shared__ float s_pb[2][kKmax], s_pnb[2][kKmax], s_tot[2][kKmax];
  __shared__ int s_last[2][kKmax], s_len[2][kKmax];
  __shared__ u64 s_hash[2][kKmax];
  __shared__ unsigned s_mk[kKmax];                           // entry k: the entries that are prefix_k + one token
  __shared__ float s_spb[kKmax], s_spnb[kKmax];              // the stay candidate's (pb', pnb') of entry k
  __shared__ float xs[kStage * kMaxThreads];                 // x[t][c] of this frame, c < kStage * threads
  __shared__ float red_v[2][kMaxThreads / 64];
  __shared__ int red_i[2][kMaxThreads / 64];
  __shared__ int2 s_hist[kHistLds];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  const int len = clamp_len(lens[b], T);
  int32_t* hypb = hyp + (int64_t)b * K * T;
  if (len == 0) {                                            // no frames: the empty hypothesis at score 0
    for (int64_t i = tid; i < (int64_t)K * T; i += nt) hypb[i] = -1;
    if (tid < K) {
      if constexpr (WLM) {
        wlm::WordPos e = wlm::start_pos(g.w);
        wlm::finish(g.w, e, 0.f, e.state, g.eos_term != 0);
        const float lm0 = e.lm;
        score[(int64_t)b * K + tid] = tid == 0 ? lm_rank(0.f, lm0, 0, g.alpha, g.beta) : -INFINITY;
        g.ctc_score[(int64_t)b * K + tid] = tid == 0 ? 0.f : -INFINITY;
        g.lm_score[(int64_t)b * K + tid] = tid == 0 ? lm0 : -INFINITY;
        g.n_words[(int64_t)b * K + tid] = tid == 0 ? 0 : -1;
      } else if constexpr (CX) {                               // (final(root) = 0: the bias of the empty hypothesis)
        float rank0 = 0.f;
        if constexpr (LM) {
          const float lm0 = g.eos >= 0 ? g.logp[(int64_t)g.start * V + g.eos] : 0.f;
          rank0 = lm_rank(0.f, lm0, 0, g.alpha, g.beta);
          g.lm_score[(int64_t)b * K + tid] = tid == 0 ? lm0 : -INFINITY;
        }
        score[(int64_t)b * K + tid] = tid == 0 ? ctx_rank(rank0, g.weight, 0.f) : -INFINITY;
        g.ctc_score[(int64_t)b * K + tid] = tid == 0 ? 0.f : -INFINITY;
        g.ctx_score[(int64_t)b * K + tid] = tid == 0 ? 0.f : -INFINITY;
      } else if constexpr (LM) {
        const float lm0 = g.eos >= 0 ? g.logp[(int64_t)g.start * V + g.eos] : 0.f;
        score[(int64_t)b * K + tid] = tid == 0 ? lm_rank(0.f, lm0, 0, g.alpha, g.beta) : -INFINITY;
        g.ctc_score[(int64_t)b * K + tid] = tid == 0 ? 0.f : -INFINITY;
        g.lm_score[(int64_t)b * K + tid] = tid == 0 ? lm0 : -INFINITY;
      } else {
        score[(int64_t)b * K + tid] = tid == 0 ? 0.f : -INFINITY;
      }
      hyp_len[(int64_t)b * K + tid] = tid == 0 ? 0 : -1;
    }
    return;
  }
  const float* zb = z + (int64_t)b * T * ld;
  const float* lse = w.lse + (int64_t)b * T;
  int2* hist = (int64_t)len * K <= kHistLds ? s_hist : w.hist + (int64_t)b * T * K;
  int croot = -1;                                            // (context) the root of this utterance's graph; < 0: no biasing
  if constexpr (CX) croot = ctx::graph_root(g.c, g.graph_of, b);
  const int nstage = kStage * nt;
  if (tid < K) {                                             // the empty prefix at (0, -inf)
    s_pb[0][tid] = tid == 0 ? 0.f : -INFINITY;
    s_pnb[0][tid] = -INFINITY;
    s_tot[0][tid] = tid == 0 ? 0.f : -INFINITY;
    s_last[0][tid] = -1;
    s_len[0][tid] = 0;
    s_hash[0][tid] = 0;
    if constexpr (LM) {
      s_state[0][tid] = g.start;
      s_lm[0][tid] = 0.f;
    }
    if constexpr (CX) {
      s_cst[0][tid] = croot;
      s_bias[0][tid] = 0.f;
    }
    if constexpr (WLM) {
      s_state[0][tid] = g.w.start;
      s_lm[0][tid] = 0.f;
      s_node[0][tid] = 0;
      s_nw[0][tid] = 0;
      s_clp[0][tid] = 0.f;
      s_cnx[0][tid] = g.w.start;
    }
  }
  float zn[kStage];
  float ln = lse[0];
#pragma unroll
  for (int i = 0; i < kStage; ++i) {
    const int c = tid + i * nt;
    zn[i] = c < V ? zb[c] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < kStage; ++i) xs[tid + i * nt] = zn[i] - ln;
  __syncthreads();
  int p = 0, nlive = 1;
  for (int t = 0; t < len; ++t) {
    const float* zr = zb + (int64_t)t * ld;
    const float lcur = ln;
    if (t + 1 < len) {                                       // the next frame's emissions: in flight while this frame runs
      ln = lse[t + 1];
#pragma unroll
      for (int i = 0; i < kStage; ++i) {
        const int c = tid + i * nt;
        if (c < V) zn[i] = zr[ld + c];
      }
    }
    // the merge map
    if (tid < nlive) {
      const u64 hj = s_hash[p][tid];
      const int lj = s_len[p][tid];
      unsigned mk = 0;
      for (int i = 0; i < nlive; ++i)
        if (s_len[p][i] == lj + 1 && prefix_hash(hj, s_last[p][i]) == s_hash[p][i]) mk |= 1u << i;
      s_mk[tid] = mk;
    }
    __syncthreads();
    float lv[M];
    int li[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
      lv[j] = -INFINITY;
      li[j] = INT_MAX;
    }
    // the stay candidate of entry tid (flat index tid: the lowest of this thread's candidates)
    if (tid < nlive) {
      const int cj = s_last[p][tid], lj = s_len[p][tid];
      const u64 hj = s_hash[p][tid];
      const float x0 = xs[0];
      const float xj = cj < 0 ? 0.f : (cj < nstage ? xs[cj] : zr[cj] - lcur);
      const float npb = s_tot[p][tid] + x0;
      float npnb = cj < 0 ? -INFINITY : s_pnb[p][tid] + xj;
      for (int i = 0; i < nlive; ++i)                        // prefix_i . cj is this entry: its mass joins here
        if (cj >= 0 && s_len[p][i] + 1 == lj && prefix_hash(s_hash[p][i], cj) == hj)
          npnb = logaddexp(npnb, (s_last[p][i] == cj ? s_pb[p][i] : s_tot[p][i]) + xj);
      s_spb[tid] = npb;
      s_spnb[tid] = npnb;
      if constexpr (CX) {
        const float st = logaddexp(npb, npnb);
        s_stot[tid] = st;
        float rk = st;
        if constexpr (LM) rk = lm_rank(st, s_lm[p][tid], lj, g.alpha, g.beta);
        top_insert(lv, li, ctx_rank(rk, g.weight, s_bias[p][tid]), tid);
      } else if constexpr (LM) {
        const float st = logaddexp(npb, npnb);
        s_stot[tid] = st;
        top_insert(lv, li, lm_rank(st, s_lm[p][tid], lj, g.alpha, g.beta), tid);
      } else if constexpr (WLM) {
        const float st = logaddexp(npb, npnb);
        s_stot[tid] = st;
        top_insert(lv, li, lm_rank(st, s_lm[p][tid], s_nw[p][tid], g.alpha, g.beta), tid);
      } else {
        top_insert(lv, li, logaddexp(npb, npnb), tid);
      }
    }
    // the extensions, entry-major
    for (int k = 0; k < nlive; ++k) {
      const int ck = s_last[p][k];
      const float pbk = s_pb[p][k], totk = s_tot[p][k];
      const unsigned mkk = s_mk[k];
      const int base = K + k * (V - 1) - 1;
      float lmk = 0.f;
      const float* lrow = nullptr;
      int lenk1 = 0;
      if constexpr (LM) {
        lmk = s_lm[p][k];
        lrow = g.logp + (int64_t)s_state[p][k] * V;
        lenk1 = s_len[p][k] + 1;
      }
      // (word LM) what an extension by <space> and by any other token carry: only a <space> behind a pending word closes it
      float lm_sp = 0.f;
      int nwk = 0, nw_sp = 0;
      bool no_sp = false;
      const int32_t* trow = nullptr;
      if constexpr (WLM) {
        const int nodek = s_node[p][k];
        lmk = s_lm[p][k];
        nwk = s_nw[p][k];
        lm_sp = nodek != 0 ? __fadd_rn(lmk, s_clp[p][k]) : lmk;
        nw_sp = nodek != 0 ? nwk + 1 : nwk;
        if (g.lexicon_only) {                                    // (the node of an entry is never off the trie then)
          no_sp = nodek != 0 && s_cnx[p][k] < 0;
          trow = g.w.trie_next + (int64_t)nodek * V;
        }
      }
      // (context) what the transitions of the entry's state share, and its bias
      ctx::Node cnode{};
      float biask = 0.f;
      if constexpr (CX) {
        if (croot >= 0) cnode = ctx::node(g.c, s_cst[p][k]);
        biask = s_bias[p][k];
      }
      for (int c = tid; c < V; c += nt) {
        if (c == 0) continue;
        const float xc = c < nstage ? xs[c] : zr[c] - lcur;
        float val = (c == ck ? pbk : totk) + xc;
        for (unsigned m = mkk; m; m &= m - 1)                // prefix_k . c is in the beam: not a candidate of its own
          if (s_last[p][__ffs(m) - 1] == c) val = -INFINITY;
        if constexpr (LM) val = lm_rank(val, lmk + lrow[c], lenk1, g.alpha, g.beta);       // (-inf stays -inf: lm is finite)
        if constexpr (WLM) {
          const bool sp = c == g.w.space;
          if (g.lexicon_only && (sp ? no_sp : trow[c] < 0)) val = -INFINITY;
          val = lm_rank(val, sp ? lm_sp : lmk, sp ? nw_sp : nwk, g.alpha, g.beta);
        }
        if constexpr (CX) {                                      // (-inf stays -inf: weight and bias are finite)
          float nb = biask;
          if (croot >= 0) {
            float d;
            ctx::arc(g.c, cnode, c, &d);
            nb = __fadd_rn(biask, d);
          }
          val = ctx_rank(val, g.weight, nb);
        }
        top_insert(lv, li, val, base + c);
      }
    }
    // select: K rounds of the workgroup arg-best over the list heads; the owner of the winner pops its head.  The list's clear
    // above, the round and the pop are seq_common.h's top_clear / top_round / top_pop_if_head spelled out: this loop runs K
    // times per frame on the serial chain, and through the helpers the compiler gives it another shape
    int nsel = 0, my_i = INT_MAX;
    float my_v = -INFINITY;
    for (int r = 0; r < K; ++r) {
      float v = lv[0];
      int i = li[0];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        if (better(ov, oi, v, i)) {
          v = ov;
          i = oi;
        }
      }
      if (nw > 1) {                                          // (uniform) double-buffered: one barrier per round
        const int buf = r & 1;
        if (lane == 0) {
          red_v[buf][wave] = v;
          red_i[buf][wave] = i;
        }
        __syncthreads();
        v = red_v[buf][0];
        i = red_i[buf][0];
        for (int ww = 1; ww < nw; ++ww)
          if (better(red_v[buf][ww], red_i[buf][ww], v, i)) {
            v = red_v[buf][ww];
            i = red_i[buf][ww];
          }
      }
      if (v == -INFINITY) break;                             // fewer than K candidates above -inf (uniform)
      if (li[0] == i) {
#pragma unroll
        for (int j = 0; j < M - 1; ++j) {
          lv[j] = lv[j + 1];
          li[j] = li[j + 1];
        }
        lv[M - 1] = -INFINITY;
        li[M - 1] = INT_MAX;
      }
      if (tid == r) {
        my_v = v;
        my_i = i;
      }
      nsel = r + 1;
    }
    __syncthreads();                                         // every read of xs and of slot p's candidates is done
    // update: entry tid of the other slot, and the frame's history
    const int q = p ^ 1;
    if (tid < K) {
      if (tid < nsel) {
        int k, tok;
        if (my_i < K) {
          k = my_i, tok = 0;
          s_pb[q][tid] = s_spb[k];
          s_pnb[q][tid] = s_spnb[k];
          s_last[q][tid] = s_last[p][k];
          s_len[q][tid] = s_len[p][k];
          s_hash[q][tid] = s_hash[p][k];
          if constexpr (RK) s_tot[q][tid] = s_stot[k];
          if constexpr (LM || WLM) {
            s_lm[q][tid] = s_lm[p][k];
            s_state[q][tid] = s_state[p][k];
          }
          if constexpr (CX) {
            s_cst[q][tid] = s_cst[p][k];
            s_bias[q][tid] = s_bias[p][k];
          }
          if constexpr (WLM) {
            s_node[q][tid] = s_node[p][k];
            s_nw[q][tid] = s_nw[p][k];
            s_clp[q][tid] = s_clp[p][k];
            s_cnx[q][tid] = s_cnx[p][k];
          }
        } else {
          const int e = my_i - K;
          k = e / (V - 1), tok = e - k * (V - 1) + 1;
          s_pb[q][tid] = -INFINITY;
          if constexpr (CX) {                                    // the winner's state and bias once more: the walk's step
            int cs = s_cst[p][k];
            float nb = s_bias[p][k];
            if (croot >= 0) {
              float d;
              cs = ctx::step(g.c, cs, tok, &d);
              nb = __fadd_rn(nb, d);
            }
            s_cst[q][tid] = cs;
            s_bias[q][tid] = nb;
            if constexpr (!LM) {                                 // my_v is a rank: the candidate's mass once more
              const float xc = tok < nstage ? xs[tok] : zr[tok] - lcur;
              const float mass = (tok == s_last[p][k] ? s_pb[p][k] : s_tot[p][k]) + xc;
              s_pnb[q][tid] = mass;
              s_tot[q][tid] = mass;
            }
          }
          if constexpr (LM) {                                    // my_v is a rank: the candidate's mass once more
            const float xc = tok < nstage ? xs[tok] : zr[tok] - lcur;
            const float mass = (tok == s_last[p][k] ? s_pb[p][k] : s_tot[p][k]) + xc;
            const int64_t at = (int64_t)s_state[p][k] * V + tok;
            s_pnb[q][tid] = mass;
            s_tot[q][tid] = mass;
            s_lm[q][tid] = s_lm[p][k] + g.logp[at];
            s_state[q][tid] = g.next[at];
          } else if constexpr (WLM) {
            const float xc = tok < nstage ? xs[tok] : zr[tok] - lcur;
            const float mass = (tok == s_last[p][k] ? s_pb[p][k] : s_tot[p][k]) + xc;
            s_pnb[q][tid] = mass;
            s_tot[q][tid] = mass;
            const wlm::WordPos e = wlm::after_token(g.w, wlm::WordPos{s_node[p][k], s_state[p][k], s_lm[p][k], s_nw[p][k]}, tok,
                                                    s_clp[p][k], s_cnx[p][k]);
            float cl;
            int cn;
            wlm::close_pair(g.w, e.node, e.state, g.lexicon_only != 0, cl, cn);               // the new entry's close pair, once
            s_lm[q][tid] = e.lm;
            s_state[q][tid] = e.state;
            s_node[q][tid] = e.node;
            s_nw[q][tid] = e.nw;
            s_clp[q][tid] = cl;
            s_cnx[q][tid] = cn;
          } else if constexpr (!CX) {
            s_pnb[q][tid] = my_v;
          }
          s_last[q][tid] = tok;
          s_len[q][tid] = s_len[p][k] + 1;
          s_hash[q][tid] = prefix_hash(s_hash[p][k], tok);
        }
        if constexpr (!RK) s_tot[q][tid] = my_v;
        hist[(int64_t)t * K + tid] = make_int2(k, tok);
      } else {
        s_tot[q][tid] = -INFINITY;
      }
    }
    if constexpr (RK) __syncthreads();                         // update has read xs
    if (t + 1 < len) {
#pragma unroll
      for (int i = 0; i < kStage; ++i) xs[tid + i * nt] = zn[i] - ln;
    }
    __syncthreads();
    p = q;
    nlive = nsel;
  }
  // The n-gram mode keeps a tail of its own, with its ranks and positions in s_rank / s_pos: folded into the tail below it
  // measured about 1 % slower at K = 4 (0.6948 -> 0.7011 ms at B = 32, T' = 100, V = 50), and the fold gave way.
  if constexpr (LM || CX) {
    // (context: final of the state joins bias, and weight bias the rank, in the same way)
    // the end-of-sentence term joins lm; the entries rank by lm_rank once more, ties to the search's order (without the term
    // every rank is the select's and the order stays); thread r walks the history of entry r back into the row of its rank
    if (tid < nlive) {
      float rk = s_tot[p][tid];
      if constexpr (LM) {
        float lm = s_lm[p][tid];
        if (g.eos >= 0) lm += g.logp[(int64_t)s_state[p][tid] * V + g.eos];
        s_lm[p][tid] = lm;
        rk = lm_rank(s_tot[p][tid], lm, s_len[p][tid], g.alpha, g.beta);
      }
      if constexpr (CX) {
        float bias = s_bias[p][tid];
        if (croot >= 0) bias = ctx::finish(g.c, s_cst[p][tid], bias);
        s_bias[p][tid] = bias;
        rk = ctx_rank(rk, g.weight, bias);
      }
      s_rank[tid] = rk;
    }
    __syncthreads();
    if (tid < K) {
      int at = tid;
      if (tid < nlive) {
        const float rv = s_rank[tid];
        at = 0;
        for (int j = 0; j < nlive; ++j) at += j != tid && better(s_rank[j], j, rv, tid) ? 1 : 0;
        int32_t* row = hypb + (int64_t)at * T;
        const int n = s_len[p][tid];
        int pos = n - 1, slot = tid;
        for (int t = len - 1; t >= 0; --t) {
          const int2 e = hist[(int64_t)t * K + slot];
          if (e.y != 0 && pos >= 0) row[pos--] = e.y;
          slot = e.x;
        }
        score[(int64_t)b * K + at] = rv;
        g.ctc_score[(int64_t)b * K + at] = s_tot[p][tid];
        if constexpr (LM) g.lm_score[(int64_t)b * K + at] = s_lm[p][tid];
        if constexpr (CX) g.ctx_score[(int64_t)b * K + at] = s_bias[p][tid];
        hyp_len[(int64_t)b * K + at] = n;
      } else {
        score[(int64_t)b * K + tid] = -INFINITY;
        g.ctc_score[(int64_t)b * K + tid] = -INFINITY;
        if constexpr (LM) g.lm_score[(int64_t)b * K + tid] = -INFINITY;
        if constexpr (CX) g.ctx_score[(int64_t)b * K + tid] = -INFINITY;
        hyp_len[(int64_t)b * K + tid] = -1;
      }
      s_pos[tid] = at;
    }
    __syncthreads();
    for (int r = 0; r < K; ++r) {
      const int n = r < nlive ? s_len[p][r] : 0;
      for (int i = n + tid; i < T; i += nt) hypb[(int64_t)s_pos[r] * T + i] = -1;
    }
    return;
  }
  // the score rows of list position `at`: a hypothesis of n tokens, or (n = -1, everything else -inf / -1) an unused slot
  const auto put = [&](int at, int n, float rank, float tot, float lm, int words) {
    const int64_t o = (int64_t)b * K + at;
    score[o] = rank;
    hyp_len[o] = n;
    if constexpr (RK) {
      g.ctc_score[o] = tot;
      g.lm_score[o] = lm;
    }
    if constexpr (WLM) g.n_words[o] = words;
  };
  const auto put_unused = [&](int at) { put(at, -1, -INFINITY, -INFINITY, -INFINITY, -1); };
  // The tail of the plain and the word-LM mode.  Plain: the beam IS the ranking - entry tid goes to row tid at rank tot.  With
  // the word LM inside, entry tid first becomes a complete hypothesis (wlm::finish: its pending word closes, then the
  // end-of-sentence term joins lm) and the (at most K) entries rank by lm_rank once more, ties to the search's order.  With
  // lexicon_only an entry whose pending node ends no word leaves the list: rank -inf, behind every other, an unused slot.
  // s_spb and s_mk are dead after the last frame: they hold the ranks and the positions.
  float* const s_rk = s_spb;
  int* const s_at = (int*)s_mk;
  float rank = -INFINITY, lm = 0.f;
  int at = tid, words = 0;
  if (tid < nlive) {
    rank = s_tot[p][tid];
    if constexpr (WLM) {
      wlm::WordPos e{s_node[p][tid], s_state[p][tid], s_lm[p][tid], s_nw[p][tid]};
      const bool ok = wlm::finish(g.w, e, s_clp[p][tid], s_cnx[p][tid], g.eos_term != 0);
      lm = e.lm, words = e.nw;
      rank = ok ? lm_rank(rank, lm, words, g.alpha, g.beta) : -INFINITY;
    }
    if constexpr (WLM) s_rk[tid] = rank;
  }
  if constexpr (WLM) {
    __syncthreads();
    if (tid < nlive) {
      at = 0;
      for (int j = 0; j < nlive; ++j) at += j != tid && better(s_rk[j], j, rank, tid) ? 1 : 0;
    }
    if (tid < K) s_at[tid] = at;
  }
  const auto kept = [&](int r, float rk) { return r < nlive && (!WLM || rk != -INFINITY); };      // entry r is a hypothesis
  if (tid < K) {
    if (kept(tid, rank)) {                                   // the history of entry tid, walked back into the row of its rank
      int32_t* row = hypb + (int64_t)at * T;
      const int n = s_len[p][tid];
      int pos = n - 1, slot = tid;
      for (int t = len - 1; t >= 0; --t) {
        const int2 e = hist[(int64_t)t * K + slot];
        if (e.y != 0 && pos >= 0) row[pos--] = e.y;
        slot = e.x;
      }
      put(at, n, rank, s_tot[p][tid], lm, words);
    } else {
      put_unused(at);
    }
  }
  if constexpr (WLM) __syncthreads();
  for (int r = 0; r < K; ++r) {
    const int n = kept(r, WLM ? s_rk[r] : 0.f) ? s_len[p][r] : 0;
    for (int i = n + tid; i < T; i += nt) hypb[(int64_t)(WLM ? s_at[r] : r) * T + i] = -1;
  }
}

int beam_check(int B, int T, int V, int K) {
  if (B <= 0 || T <= 0 || V <= 0) return ASR_E_ARG;
  if (V < 2 || K < 1 || K > kKmax || (int64_t)K * V > INT_MAX / 2 || ((int64_t)B * T + kLseWaves - 1) / kLseWaves > 0x7fffffffLL)
    return ASR_E_SHAPE;
  return 0;
}

// what the four entries check first, and what they do once their own checks have passed
bool common_args_ok(const float* logits, int64_t ld, int V, const int32_t* frame_lens, const int32_t* hyp, const int32_t* hyp_len,
                    const float* score, const void* ws) {
  return logits && frame_lens && hyp && hyp_len && score && ws && ld >= V;
}

template <int MODE, class G>
int launch(int B, int T, int V, int K, const float* logits, int64_t ld, const int32_t* frame_lens, int32_t* hyp, int32_t* hyp_len,
           float* score, void* ws, const G& g, hipStream_t stream) {
  if ((((uintptr_t)ws) & 7u) != 0) return ASR_E_ALIGN;
  const BeamWs w = beam_ws(ws, B, T, K);
  launch_frame_lse(B, T, V, logits, ld, frame_lens, w.lse, stream);
  ASR_CHECK_LAUNCH();
  const dim3 grid(B), block((int64_t)K * V <= kOneWaveKV ? 64 : kMaxThreads);
#define CTC_BEAM(M_) \
  hipLaunchKernelGGL((ctc_beam_kernel<M_, MODE>), grid, block, 0, stream, T, V, K, logits, ld, frame_lens, hyp, hyp_len, score, w, g)
  if (K <= 1) CTC_BEAM(1);
  else if (K <= 2) CTC_BEAM(2);
  else if (K <= 4) CTC_BEAM(4);
  else if (K <= 8) CTC_BEAM(8);
  else CTC_BEAM(16);
#undef CTC_BEAM
  ASR_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int asr_ctc_beam_ws_bytes(int B, int T, int V, int K, int64_t* ws_bytes) {
  if (!ws_bytes) return ASR_E_ARG;
  const int rc = beam_check(B, T, V, K);
  if (rc) return rc;
  *ws_bytes = beam_ws(nullptr, B, T, K).bytes;
  return 0;
}

extern "C" int asr_ctc_beam_f32(int B, int T, int V, int K, const float* logits, int64_t ld, const int32_t* frame_lens,
                                int32_t* hyp, int32_t* hyp_len, float* score, void* ws, asr_stream_t stream) {
  if (!common_args_ok(logits, ld, V, frame_lens, hyp, hyp_len, score, ws)) return ASR_E_ARG;
  const int rc = beam_check(B, T, V, K);
  if (rc) return rc;
  return launch<kPlain>(B, T, V, K, logits, ld, frame_lens, hyp, hyp_len, score, ws, BeamLm{}, (hipStream_t)stream);
}

extern "C" int asr_ctc_beam_lm_f32(int B, int T, int V, int K, const float* logits, int64_t ld, const int32_t* frame_lens, int S,
                                   const float* lm_logp, const int32_t* lm_next, int lm_start, int lm_eos, float alpha, float beta,
                                   int32_t* hyp, int32_t* hyp_len, float* score, float* ctc_score, float* lm_score, void* ws,
                                   asr_stream_t stream) {
  if (!common_args_ok(logits, ld, V, frame_lens, hyp, hyp_len, score, ws) || !lm_logp || !lm_next || !ctc_score || !lm_score ||
      S <= 0 || !(fabsf(alpha) <= FLT_MAX) || !(fabsf(beta) <= FLT_MAX))
    return ASR_E_ARG;
  const int rc = beam_check(B, T, V, K);
  if (rc) return rc;
  if ((int64_t)S * V > INT_MAX || lm_start < 0 || lm_start >= S || lm_eos >= V) return ASR_E_SHAPE;
  BeamLm g;
  g.logp = lm_logp, g.next = lm_next, g.ctc_score = ctc_score, g.lm_score = lm_score;
  g.start = lm_start, g.eos = lm_eos < 0 ? -1 : lm_eos, g.alpha = alpha, g.beta = beta;
  return launch<kNgram>(B, T, V, K, logits, ld, frame_lens, hyp, hyp_len, score, ws, g, (hipStream_t)stream);
}

extern "C" int asr_ctc_beam_ctx_f32(int B, int T, int V, int K, const float* logits, int64_t ld, const int32_t* frame_lens,
                                    const asr_context_t* c, const int32_t* graph_of, float ctx_weight, int S, const float* lm_logp,
                                    const int32_t* lm_next, int lm_start, int lm_eos, float alpha, float beta, int32_t* hyp,
                                    int32_t* hyp_len, float* score, float* ctc_score, float* lm_score, float* ctx_score, void* ws,
                                    asr_stream_t stream) {
  if (!common_args_ok(logits, ld, V, frame_lens, hyp, hyp_len, score, ws) || !graph_of || !ctc_score || !ctx_score || S < 0 ||
      !(fabsf(ctx_weight) <= FLT_MAX))
    return ASR_E_ARG;
  if (S > 0 && (!lm_logp || !lm_next || !lm_score || !(fabsf(alpha) <= FLT_MAX) || !(fabsf(beta) <= FLT_MAX))) return ASR_E_ARG;
  int rc = ctx::check_abi(c);
  if (rc) return rc;
  rc = beam_check(B, T, V, K);
  if (rc) return rc;
  if (c->V != V) return ASR_E_SHAPE;
  if (S > 0 && ((int64_t)S * V > INT_MAX || lm_start < 0 || lm_start >= S || lm_eos >= V)) return ASR_E_SHAPE;
  BeamCtx g{};
  g.c = ctx::from_abi(*c), g.graph_of = graph_of, g.ctx_score = ctx_score, g.weight = ctx_weight;
  g.ctc_score = ctc_score;
  if (S == 0) return launch<kCtx>(B, T, V, K, logits, ld, frame_lens, hyp, hyp_len, score, ws, g, (hipStream_t)stream);
  g.logp = lm_logp, g.next = lm_next, g.lm_score = lm_score;
  g.start = lm_start, g.eos = lm_eos < 0 ? -1 : lm_eos, g.alpha = alpha, g.beta = beta;
  return launch<kNgramCtx>(B, T, V, K, logits, ld, frame_lens, hyp, hyp_len, score, ws, g, (hipStream_t)stream);
}

extern "C" int asr_ctc_beam_wlm_f32(int B, int T, int V, int K, const float* logits, int64_t ld, const int32_t* frame_lens,
                                    const asr_word_lm_t* lm, float alpha, float beta, int eos_term, int lexicon_only,
                                    int32_t* hyp, int32_t* hyp_len, float* score, float* ctc_score, float* lm_score,
                                    int32_t* n_words, void* ws, asr_stream_t stream) {
  if (!common_args_ok(logits, ld, V, frame_lens, hyp, hyp_len, score, ws) || !ctc_score || !lm_score || !n_words ||
      !(fabsf(alpha) <= FLT_MAX) || !(fabsf(beta) <= FLT_MAX))
    return ASR_E_ARG;
  int rc = wlm::check_abi(lm);
  if (rc) return rc;
  rc = beam_check(B, T, V, K);
  if (rc) return rc;
  if (lm->V != V) return ASR_E_SHAPE;
  BeamWlm g;
  g.w = wlm::from_abi(*lm);
  g.ctc_score = ctc_score, g.lm_score = lm_score, g.n_words = n_words;
  g.alpha = alpha, g.beta = beta, g.eos_term = eos_term != 0, g.lexicon_only = lexicon_only != 0;
  return launch<kWordLm>(B, T, V, K, logits, ld, frame_lens, hyp, hyp_len, score, ws, g, (hipStream_t)stream);
}
