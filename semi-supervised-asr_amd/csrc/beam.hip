// beam.hip — beam-search decoding between two decoder steps (Decoder.recognize_beams, model.py:369-406; the reference
// leaves the method unfinished, the semantics are DESIGN 4.8's).  Per step the host runs asr_dec_step_fwd and the skinny
// output GEMM on B*K rows, then:
//   beam_select   one workgroup per utterance: log-softmax of each live beam's logits, the top 2K of the K*V candidates
//                 (score desc, flat index k*V+v asc on ties), the fairseq walk over them (<EOS> at rank < K finishes a
//                 hypothesis, other <EOS> are skipped, non-<EOS> fill the live slots in rank order);
//   beam_reorder  one workgroup per beam row: the next step's input slot gathers its predecessor's z, ctx, cell state
//                 and attention weights (out of place: source and destination are different step slots) and the
//                 embedding of its new token;
// One select kernel serves every mode.  Each candidate's value is beam_base: score + logp, with a language model (shallow
// fusion) + lm_weight * log_softmax(lm_logits), with the CTC prefix score (joint CTC-attention decoding, DESIGN
// 4.15; csrc/ctc_prefix.hip computes psi) score + (1 - w) logp + w (psi - psi_prev) (+ the LM's term).  beam_reorder_lm gathers
// the LM's h / c of every layer (and the decoder's state) in one launch.
// With an n-gram automaton or a lexicon and word-level LM inside the search (KIND) the kernel ranks
// (base' + weight lm') + bonus len' (word LM: nw') where base' is beam_base: scores keeps base, the LM position of every beam
// row and the parts of the finished entries live in the caller's extra workspace, one thread per live entry does the word LM's
// lookups up front, one thread per winner forms its parts again, and the walker thread writes the new positions in place - the
// reorder kernels are used as they are.  Without such an LM none of that state exists (if constexpr, arrays of the mode's size).
// And once at the end
//   beam_backtrack  one workgroup per utterance: rank the finished hypotheses, follow the backpointers into token rows.
#include <float.h>
#include "seq_common.h"
#include "word_lm.h"

namespace {

constexpr int BEAM_NT = 256;               // threads of the select / reorder / backtrack workgroups
constexpr int BEAM_WAVES = BEAM_NT / 64;
constexpr int BEAM_KMAX = ASR_BEAM_KMAX;
constexpr int BEAM_FCAP = ASR_BEAM_FCAP;   // finished entries per utterance (< 2K can be held: include/asr_hip.h)

// CTC: the candidate carries the prefix score's term; without it the kernel has no CTC argument at all (an empty structure)
template <bool CTC>
struct beam_ctc_args {
  const float* psi;        // [B*K][V]
  const float* psi_prev;   // [B*K]
  float w;
};
template <>
struct beam_ctc_args<false> {};

// ---- an n-gram or a word-level LM inside the search ----------------------------------------------------------
// The caller's extra workspace beside asr_beam_t: the LM position of every beam row and the parts of the finished entries.
//   a / b     n-gram: the automaton state / unused;  word LM: the trie node of the pending word / the word state
//   lm, n     the LM's fp32 sum;  n-gram: the non-<EOS> tokens (len);  word LM: the completed words (nw)
// Without such an LM (TLM_NONE) the select kernel's argument is the empty structure.
constexpr int TLM_NONE = 0, TLM_NGRAM = 1, TLM_WORD = 2;
template <bool ON>
struct BeamTlm {
  const float* logp;       // n-gram: [S][V]
  const int32_t* next;
  int start;
  wlm::WordLm w;           // word LM
  float weight, bonus;
  bool lexicon_only;
  int32_t *a, *b, *n;      // [B*K] positions
  float* lm;
  float *fin_base, *fin_lm;   // [B][BEAM_FCAP] parts of the finished entries (p.fin_score holds their rank)
  int32_t* fin_n;
};
template <>
struct BeamTlm<false> {};

inline int64_t tlm_ws_bytes(int B, int K) { return 4 * (4 * round64((int64_t)B * K) + 3 * round64((int64_t)B * BEAM_FCAP)); }

// THE candidate value of every mode: score + logp, with the judge + lmw * logp_lm, with the CTC prefix score
// score + (1 - w) logp + w (psi - psi_prev) (+ lmw * logp_lm).  The rounded intrinsics are plain operators to this compiler, so
// the contraction is switched off and the two fused multiply-adds this search has always had are written out: the judge's
// product into its sum where the judge is the only extra term; with both terms, (1 - w) logp into score; none with the CTC term
// alone.  The candidate loop and the second pass over the winners both call this, so they agree, and zero weights of an LM
// inside the search reproduce the search without it (tests/test_beam_ngram_gpu.py holds both).
template <bool LM, bool CTC>
__device__ __forceinline__ float beam_base(float sc, float x, float m, float ls, float lx, float lmm, float lml, float lmw,
                                           float px, float pprev, float omw, float cw) {
#pragma clang fp contract(off)
  const float lp = (x - m) - ls;
  float c;
  if (CTC) {
    const float a = omw * lp;
    const float d = px - pprev;
    const float e = cw * d;
    c = LM ? __builtin_fmaf(omw, lp, sc) : sc + a;
    c = c + e;
  } else {
    c = sc + lp;
  }
  if (LM) {
    const float llp = (lx - lmm) - lml;
    const float f = lmw * llp;
    c = CTC ? c + f : __builtin_fmaf(lmw, llp, c);
  }
  return c;
}

// lm_rank's expression, (base + weight lm) + bonus n, with every one of the four operations rounded on its own: the rounded
// intrinsics are plain operators to this compiler, so the contraction into a fused multiply-add is switched off here
__device__ __forceinline__ float tlm_rank(float base, float lm, int n, float weight, float bonus) {
#pragma clang fp contract(off)
  const float wl = weight * lm;
  const float s = base + wl;
  const float bn = bonus * (float)n;
  return s + bn;
}

// the staged position of a live entry (LDS), with what one thread looked up for it up front
struct TlmStage {
  int a, b, n;             // the old position
  float lm;
  float clp;               // word LM: the close pair of the pending word ...
  int cnext;
  float e_lm;              // ... and the entry as a complete hypothesis: lm, words, and whether it is one (lexicon_only)
  int e_n, e_ok;
};

// lm', n' and validity of candidate v from the staged entry.  n-gram: one read of the entry's table row; word LM: LDS only,
// and with lexicon_only one read of the entry's trie_next row.
template <int KIND>
__device__ __forceinline__ bool tlm_candidate(const BeamTlm<true>& g, const TlmStage& s, int v, int V, int eos, float& lm, int& n) {
  if constexpr (KIND == TLM_NGRAM) {
    lm = __fadd_rn(s.lm, g.logp[(int64_t)s.a * V + v]);
    n = s.n + (v != eos ? 1 : 0);
    return true;
  } else {
    if (v == eos) {
      lm = s.e_lm, n = s.e_n;
      return s.e_ok != 0;
    }
    lm = s.lm, n = s.n;
    if (v == g.w.space) {
      if (s.a != 0) {
        if (s.cnext < 0) return false;                      // lexicon_only: the pending node ends no word
        lm = __fadd_rn(s.lm, s.clp), n = s.n + 1;
      }
      return true;
    }
    if (g.lexicon_only) return wlm::trie_step(g.w, s.a, v) >= 0;
    return true;
  }
}

// M: the per-thread candidate list length, a power of two >= 2K.  LM, CTC: beam_base's terms; without LM lm_logits / lmw are
// not read.  KIND: the LM inside the search; the arrays that only it needs have one element without it and, never named, take
// no LDS.
template <int M, bool LM, bool CTC, int KIND>
__global__ __launch_bounds__(BEAM_NT) void beam_select_kernel(asr_beam_t p, int t, const float* __restrict__ lm_logits,
                                                              float lmw, beam_ctc_args<CTC> ca, BeamTlm<KIND != TLM_NONE> g) {
  constexpr bool TLM = KIND != TLM_NONE;
  constexpr int NK = TLM ? BEAM_KMAX : 1, NTOP = TLM ? 2 * BEAM_KMAX : 1;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = p.K, V = p.V, B = p.B;
  if (p.done[b]) return;                                   // finished utterances are left untouched
  __shared__ float s_score[BEAM_KMAX], s_max[BEAM_KMAX], s_lsum[BEAM_KMAX];
  __shared__ float s_lmmax[LM ? BEAM_KMAX : 1], s_lmlsum[LM ? BEAM_KMAX : 1];
  __shared__ TlmStage s_pos[NK];
  __shared__ float red_v[2][BEAM_WAVES];
  __shared__ int red_i[2][BEAM_WAVES];
  __shared__ float top_v[2 * BEAM_KMAX];
  __shared__ int top_i[2 * BEAM_KMAX];
  // the parts and the new position of every ranked candidate, and the same as a hypothesis finished as it stands (t = L-1)
  __shared__ float top_base[NTOP], top_lm[NTOP], top_erank[NTOP], top_elm[NTOP];
  __shared__ int top_n[NTOP], top_a[NTOP], top_b[NTOP], top_en[NTOP], top_eok[NTOP];
  __shared__ int s_ntop, live_r[NK];
  if (tid < K) {
    const float sc = p.scores[(int64_t)b * K + tid];
    s_score[tid] = sc;
    if constexpr (TLM) {
      if (sc != -INFINITY) {                                // one thread per live entry: its position, its lookups
        const int64_t r = (int64_t)b * K + tid;
        TlmStage s;
        s.a = g.a[r], s.b = 0, s.n = g.n[r], s.lm = g.lm[r];
        s.clp = 0.f, s.cnext = 0, s.e_lm = 0.f, s.e_n = 0, s.e_ok = 1;
        if constexpr (KIND == TLM_WORD) {
          s.b = g.b[r];
          wlm::close_pair(g.w, s.a, s.b, g.lexicon_only, s.clp, s.cnext);
          wlm::WordPos q{s.a, s.b, s.lm, s.n};
          s.e_ok = wlm::finish(g.w, q, s.clp, s.cnext, true) ? 1 : 0;
          s.e_lm = q.lm, s.e_n = q.nw;
        }
        s_pos[tid] = s;
      }
    }
  }
  __syncthreads();

  // log-softmax statistics of every live beam's row: max and log(sum exp(x - max)), one wave per row
  const float* lg = p.logits + (int64_t)b * K * V;
  for (int k = wave; k < K; k += BEAM_WAVES) {
    if (s_score[k] == -INFINITY) continue;                 // wave-uniform
    float m, s;
    wave_row_max_sumexp(lg + (int64_t)k * V, V, lane, m, s);
    if (lane == 0) { s_max[k] = m; s_lsum[k] = logf(s); }
    if (LM) {
      wave_row_max_sumexp(lm_logits + ((int64_t)b * K + k) * V, V, lane, m, s);
      if (lane == 0) { s_lmmax[k] = m; s_lmlsum[k] = logf(s); }
    }
  }
  __syncthreads();

  // every thread keeps its best M candidates (value - with an LM inside, rank - desc, flat index k*V+v asc on ties), visiting
  // flat indices in increasing order
  float lv[M];
  int li[M];
  top_clear(lv, li);
  for (int k = 0; k < K; ++k) {
    const float sc = s_score[k];
    if (sc == -INFINITY) continue;
    const float m = s_max[k], ls = s_lsum[k];
    const float* row = lg + (int64_t)k * V;
    const float* lrow = LM ? lm_logits + ((int64_t)b * K + k) * V : nullptr;
    const float lmm = LM ? s_lmmax[k] : 0.f, lml = LM ? s_lmlsum[k] : 0.f;
    const float* prow = nullptr;
    float pprev = 0.f, omw = 0.f, cw = 0.f;
    if constexpr (CTC) {
      prow = ca.psi + ((int64_t)b * K + k) * V;
      pprev = ca.psi_prev[b * K + k], cw = ca.w, omw = __fsub_rn(1.f, cw);
    }
    for (int v = tid; v < V; v += BEAM_NT) {
      float c = beam_base<LM, CTC>(sc, row[v], m, ls, LM ? lrow[v] : 0.f, lmm, lml, lmw, CTC ? prow[v] : 0.f, pprev, omw, cw);
      if constexpr (TLM) {
        float lm;
        int n;
        const bool ok = tlm_candidate<KIND>(g, s_pos[k], v, V, p.eos, lm, n);
        c = ok ? tlm_rank(c, lm, n, g.weight, g.bonus) : -INFINITY;
      }
      top_insert(lv, li, c, k * V + v);
    }
  }

  // merge: 2K rounds of a workgroup arg-best over the list heads; the owner of the winner pops its head
  const int want = 2 * K;
  int ntop = 0;
  for (int r = 0; r < want; ++r) {
    float v;
    int i;
    top_round(lv[0], li[0], red_v[r & 1], red_i[r & 1], BEAM_WAVES, v, i);
    if (v == -INFINITY) break;                              // fewer than 2K finite candidates (uniform)
    top_pop_if_head(lv, li, i);
    if (tid == 0) { top_v[r] = v; top_i[r] = i; }
    ntop = r + 1;
  }
  if (tid == 0) s_ntop = ntop;
  __syncthreads();

  // an LM inside: one thread per ranked candidate forms its parts again (the same operations on the same operands: the same
  // bits) and the position behind it; at t = L-1 also what it is as a hypothesis that finishes as it stands
  if constexpr (TLM) {
    if (tid < ntop) {
      const int idx = top_i[tid];
      const int k = idx / V, v = idx - k * V;
      const TlmStage st = s_pos[k];
      const int64_t rk = (int64_t)b * K + k;
      float pprev = 0.f, omw = 0.f, cw = 0.f, px = 0.f, lx = 0.f;
      if constexpr (CTC) px = ca.psi[rk * V + v], pprev = ca.psi_prev[rk], cw = ca.w, omw = __fsub_rn(1.f, cw);
      if (LM) lx = lm_logits[rk * V + v];
      const float base = beam_base<LM, CTC>(s_score[k], lg[(int64_t)k * V + v], s_max[k], s_lsum[k], lx, LM ? s_lmmax[k] : 0.f,
                                            LM ? s_lmlsum[k] : 0.f, lmw, px, pprev, omw, cw);
      float lm;
      int n;
      tlm_candidate<KIND>(g, st, v, V, p.eos, lm, n);
      top_base[tid] = base, top_lm[tid] = lm, top_n[tid] = n;
      int na = 0, nb = 0, eok = 1, en = n;
      float elm = lm;
      if (v != p.eos) {
        if constexpr (KIND == TLM_NGRAM) {
          na = g.next[(int64_t)st.a * V + v];
          if (t == p.L - 1) elm = __fadd_rn(lm, g.logp[(int64_t)na * V + p.eos]);
        } else {
          const wlm::WordPos q = wlm::after_token(g.w, wlm::WordPos{st.a, st.b, st.lm, st.n}, v, st.clp, st.cnext);
          na = q.node, nb = q.state;
          if (t == p.L - 1) {
            float lp;
            int nx;
            wlm::close_pair(g.w, q.node, q.state, g.lexicon_only, lp, nx);
            wlm::WordPos e = q;
            eok = wlm::finish(g.w, e, lp, nx, true) ? 1 : 0;
            elm = e.lm, en = e.nw;
          }
        }
      }
      top_a[tid] = na, top_b[tid] = nb;
      top_elm[tid] = elm, top_en[tid] = en, top_eok[tid] = eok;
      top_erank[tid] = tlm_rank(base, elm, en, g.weight, g.bonus);
    }
    __syncthreads();
  }
  if (tid != 0) return;

  // the fairseq walk over the ranked candidates (a handful of entries: one thread).  An LM inside: scores keeps base, the
  // finished list the rank and the parts, the positions move in place
  ntop = s_ntop;
  const int64_t hb = ((int64_t)t * B + b) * K;
  int nf = p.nfin[b], nlive = 0;
  for (int r = 0; r < ntop; ++r) {
    const int idx = top_i[r];
    const int k = idx / V, v = idx - k * V;
    if (v == p.eos) {
      if (r < K) {
        const int64_t fo = (int64_t)b * BEAM_FCAP + nf;
        int4* f = reinterpret_cast<int4*>(p.fin) + fo;
        *f = make_int4(t, k, t + 1, 1);
        p.fin_score[fo] = top_v[r];
        if constexpr (TLM) g.fin_base[fo] = top_base[r], g.fin_lm[fo] = top_lm[r], g.fin_n[fo] = top_n[r];
        ++nf;
      }
    } else if (nlive < K) {
      const int64_t o = (int64_t)b * K + nlive;
      p.tok_hist[hb + nlive] = v;
      p.bp_hist[hb + nlive] = k;
      if constexpr (TLM) {
        p.scores[o] = top_base[r];
        g.a[o] = top_a[r], g.lm[o] = top_lm[r], g.n[o] = top_n[r];
        if constexpr (KIND == TLM_WORD) g.b[o] = top_b[r];
        live_r[nlive] = r;
      } else {
        p.scores[o] = top_v[r];
      }
      ++nlive;
    }
  }
  for (int j = nlive; j < K; ++j) {                         // dead slots: a valid token and predecessor, score -inf
    p.tok_hist[hb + j] = p.eos;
    p.bp_hist[hb + j] = 0;
    p.scores[(int64_t)b * K + j] = -INFINITY;
  }
  if (t == p.L - 1 && nf < K) {                             // max_dec_timesteps: the live beams finish as they stand; an LM
    for (int j = 0; j < nlive; ++j) {                       // inside adds the end term an <EOS> would give and no <EOS> token
      if constexpr (TLM) {
        if (!top_eok[live_r[j]]) continue;                  // lexicon_only: the pending node ends no word
      }
      const int64_t fo = (int64_t)b * BEAM_FCAP + nf;
      int4* f = reinterpret_cast<int4*>(p.fin) + fo;
      *f = make_int4(t, j, t + 1, 0);
      if constexpr (TLM) {
        const int r = live_r[j];
        p.fin_score[fo] = top_erank[r];
        g.fin_base[fo] = top_base[r], g.fin_lm[fo] = top_elm[r], g.fin_n[fo] = top_en[r];
      } else {
        p.fin_score[fo] = p.scores[(int64_t)b * K + j];
      }
      ++nf;
    }
  }
  p.nfin[b] = nf;
  if (nf >= K || t == p.L - 1 || nlive == 0) {
    p.done[b] = 1;
    atomicAdd(p.ndone, 1);
  }
}

// the position of the empty sequence in every beam row
template <int KIND>
__global__ __launch_bounds__(BEAM_NT) void beam_tlm_init_kernel(int R, BeamTlm<true> g) {
  const int r = blockIdx.x * BEAM_NT + threadIdx.x;
  if (r >= R) return;
  g.lm[r] = 0.f, g.n[r] = 0;
  if constexpr (KIND == TLM_NGRAM) {
    g.a[r] = g.start, g.b[r] = 0;
  } else {
    const wlm::WordPos q = wlm::start_pos(g.w);
    g.a[r] = q.node, g.b[r] = q.state;
  }
}

// the decoder state of beam row `row` (not done): gathered from row `src`, with the embedding of token `tok`
__device__ __forceinline__ void beam_reorder_row(const asr_beam_state_t& s, int row, int src, int tok) {
  const int DO = s.D + s.O;
  const float* xs = s.x_src + (int64_t)src * s.ldx;
  float* xd = s.x_dst + (int64_t)row * s.ldx;
  for (int i = threadIdx.x; i < DO; i += BEAM_NT) xd[i] = xs[i];
  const float* e = s.emb + (int64_t)tok * s.E;
  for (int i = threadIdx.x; i < s.E; i += BEAM_NT) xd[DO + i] = e[i];
  for (int i = threadIdx.x; i < s.D; i += BEAM_NT) s.c_dst[(int64_t)row * s.D + i] = s.c_src[(int64_t)src * s.D + i];
  for (int i = threadIdx.x; i < s.Tp; i += BEAM_NT) s.w_dst[(int64_t)row * s.Tp + i] = s.w_src[(int64_t)src * s.Tp + i];
}

__global__ __launch_bounds__(BEAM_NT) void beam_reorder_kernel(asr_beam_t p, int t, asr_beam_state_t s) {
  const int row = blockIdx.x, b = row / p.K, j = row - b * p.K;
  if (p.done[b]) return;
  const int64_t h = ((int64_t)t * p.B + b) * p.K + j;
  beam_reorder_row(s, row, b * p.K + p.bp_hist[h], p.tok_hist[h]);
}

// blockIdx.y = 0: the decoder state (if has_dec); 1 + l: LM layer l - the h part of its input row and its cell state
// gathered by the backpointer, and for layer 0 the new token's LM embedding into the x part
__global__ __launch_bounds__(BEAM_NT) void beam_reorder_lm_kernel(asr_beam_t p, int t, asr_beam_state_t s, int has_dec,
                                                                 asr_beam_lm_state_t m) {
  const int row = blockIdx.x, b = row / p.K, j = row - b * p.K;
  if (p.done[b]) return;
  const int64_t h = ((int64_t)t * p.B + b) * p.K + j;
  const int src = b * p.K + p.bp_hist[h];
  const int tok = p.tok_hist[h];
  if (blockIdx.y == 0) {
    if (has_dec) beam_reorder_row(s, row, src, tok);
    return;
  }
  const int l = blockIdx.y - 1, H = m.H, In = m.in_dim[l];
  const int64_t ld = In + H;
  const float* hs = m.x_src[l] + (int64_t)src * ld + In;
  float* xd = m.x_dst[l] + (int64_t)row * ld;
  for (int i = threadIdx.x; i < H; i += BEAM_NT) xd[In + i] = hs[i];
  const float* cs = m.c_src[l] + (int64_t)src * H;
  float* cd = m.c_dst[l] + (int64_t)row * H;
  for (int i = threadIdx.x; i < H; i += BEAM_NT) cd[i] = cs[i];
  if (l == 0) {
    const float* e = m.emb + (int64_t)tok * In;
    for (int i = threadIdx.x; i < In; i += BEAM_NT) xd[i] = e[i];
  }
}

// PARTS: the parts of the finished entries (a search with an n-gram or word LM inside) follow the hypotheses
// into the final order; without them the structure is empty and the kernel is the plain backtrack
template <bool PARTS>
struct beam_parts_args {
  const float *fin_base, *fin_lm;   // [B][BEAM_FCAP]
  const int32_t* fin_n;
  float *out_base, *out_lm;         // [B][K]
  int32_t* out_n;
};
template <>
struct beam_parts_args<false> {};

template <bool PARTS>
__global__ __launch_bounds__(BEAM_NT) void beam_backtrack_kernel(asr_beam_t p, float alpha, int32_t* out_tok,
                                                                 float* out_score, int32_t* out_len, beam_parts_args<PARTS> pa) {
  const int b = blockIdx.x, tid = threadIdx.x, K = p.K, L = p.L;
  __shared__ int order[BEAM_FCAP];
  __shared__ float key[BEAM_FCAP];
  __shared__ int s_nf;
  const int4* fin = reinterpret_cast<const int4*>(p.fin) + (int64_t)b * BEAM_FCAP;
  if (tid == 0) {
    int nf = p.nfin[b];
    nf = nf < 0 ? 0 : (nf > BEAM_FCAP ? BEAM_FCAP : nf);
    // insertion sort by score / len^alpha, descending; stable, so ties keep the order of finishing
    for (int i = 0; i < nf; ++i) {
      const float sc = p.fin_score[(int64_t)b * BEAM_FCAP + i];
      const float kv = alpha == 0.f ? sc : sc / powf((float)fin[i].z, alpha);
      int j = i;
      while (j > 0 && kv > key[j - 1]) { key[j] = key[j - 1]; order[j] = order[j - 1]; --j; }
      key[j] = kv;
      order[j] = i;
    }
    s_nf = nf;
  }
  __syncthreads();
  const int nf = s_nf;
  for (int r = tid; r < K; r += BEAM_NT) {
    int32_t* row = out_tok + ((int64_t)b * K + r) * L;
    for (int s = 0; s < L; ++s) row[s] = p.eos;
    if (r >= nf) {
      out_score[(int64_t)b * K + r] = -INFINITY;
      out_len[(int64_t)b * K + r] = 0;
      if constexpr (PARTS) {
        pa.out_base[(int64_t)b * K + r] = -INFINITY;
        pa.out_lm[(int64_t)b * K + r] = -INFINITY;
        pa.out_n[(int64_t)b * K + r] = -1;
      }
      continue;
    }
    const int4 f = fin[order[r]];                          // (step, slot, length, ends with <EOS>)
    if constexpr (PARTS) {
      const int64_t fo = (int64_t)b * BEAM_FCAP + order[r];
      pa.out_base[(int64_t)b * K + r] = pa.fin_base[fo];
      pa.out_lm[(int64_t)b * K + r] = pa.fin_lm[fo];
      pa.out_n[(int64_t)b * K + r] = pa.fin_n[fo];
    }
    int s = f.x, j = f.y;
    if (f.w) {
      --s;                                                  // row[f.x] is the <EOS>; slot j is the beam at step f.x - 1
    }
    for (; s >= 0; --s) {
      const int64_t h = ((int64_t)s * p.B + b) * K + j;
      row[s] = p.tok_hist[h];
      j = p.bp_hist[h];
    }
    out_score[(int64_t)b * K + r] = key[r];
    out_len[(int64_t)b * K + r] = f.z;
  }
}

int check_beam(const asr_beam_t* p, bool need_logits) {
  if (!p || (need_logits && !p->logits) || !p->scores || !p->tok_hist || !p->bp_hist || !p->fin || !p->fin_score || !p->nfin || !p->done ||
      !p->ndone)
    return ASR_E_ARG;
  if (p->B <= 0 || p->K <= 0 || p->V <= 0 || p->L <= 0) return ASR_E_ARG;
  if (p->K > BEAM_KMAX || p->V < 2 || (int64_t)p->K * p->V > INT_MAX / 2 || p->eos < 0 || p->eos >= p->V) return ASR_E_SHAPE;
  if (!asr_aligned16(p->fin)) return ASR_E_ALIGN;
  return 0;
}

// the checks every select entry shares, each written once; an entry calls them in its own order of precedence
int check_step(const asr_beam_t* p, int t) {
  const int rc = check_beam(p, true);
  if (rc) return rc;
  return t < 0 || t >= p->L ? ASR_E_ARG : 0;
}

int check_ctc(const asr_beam_t* p, const float* psi, const float* psi_prev, float cw) {
  if (!(cw >= 0.f && cw <= 1.f)) return ASR_E_ARG;
  if (cw == 0.f) return 0;                                  // psi is not read: the variant without it
  if (!psi || !psi_prev) return ASR_E_ARG;
  return p && p->V < 3 ? ASR_E_SHAPE : 0;
}

// the one launch of a checked select: the judge if lm_logits, the CTC term if cw != 0, the LM inside the search if g
template <bool LM, bool CTC, int KIND>
int beam_select_launch(const asr_beam_t* p, int t, const float* lm_logits, float lmw, const float* psi, const float* psi_prev,
                       float cw, const BeamTlm<true>* g, hipStream_t stream) {
  const dim3 grid(p->B), block(BEAM_NT);
  const int m = 2 * p->K;
  beam_ctc_args<CTC> ca;
  if constexpr (CTC) ca.psi = psi, ca.psi_prev = psi_prev, ca.w = cw;
  BeamTlm<KIND != TLM_NONE> ga;
  if constexpr (KIND != TLM_NONE) ga = *g;
#define BEAM_SELECT(M_) \
  hipLaunchKernelGGL((beam_select_kernel<M_, LM, CTC, KIND>), grid, block, 0, stream, *p, t, lm_logits, lmw, ca, ga)
  if (m <= 2) BEAM_SELECT(2);
  else if (m <= 4) BEAM_SELECT(4);
  else if (m <= 8) BEAM_SELECT(8);
  else if (m <= 16) BEAM_SELECT(16);
  else BEAM_SELECT(32);
#undef BEAM_SELECT
  ASR_CHECK_LAUNCH();
  return 0;
}

int beam_select(const asr_beam_t* p, int t, const float* lm_logits, float lmw, const float* psi, const float* psi_prev, float cw,
                int kind, const BeamTlm<true>* g, hipStream_t stream) {
#define BEAM_MODE(LM_, CTC_)                                                                                            \
  (kind == TLM_WORD    ? beam_select_launch<LM_, CTC_, TLM_WORD>(p, t, lm_logits, lmw, psi, psi_prev, cw, g, stream)    \
   : kind == TLM_NGRAM ? beam_select_launch<LM_, CTC_, TLM_NGRAM>(p, t, lm_logits, lmw, psi, psi_prev, cw, g, stream)   \
                       : beam_select_launch<LM_, CTC_, TLM_NONE>(p, t, lm_logits, lmw, psi, psi_prev, cw, g, stream))
  if (cw != 0.f) return lm_logits ? BEAM_MODE(true, true) : BEAM_MODE(false, true);
  return lm_logits ? BEAM_MODE(true, false) : BEAM_MODE(false, false);
#undef BEAM_MODE
}

int check_beam_state(const asr_beam_t* p, int t, const asr_beam_state_t* s) {
  if (!s || !s->x_src || !s->x_dst || !s->c_src || !s->c_dst || !s->w_src || !s->w_dst || !s->emb) return ASR_E_ARG;
  if (t < 0 || t >= p->L || s->D <= 0 || s->O < 0 || s->E <= 0 || s->Tp <= 0 || s->ldx < s->D + s->O + s->E)
    return ASR_E_ARG;
  if (s->x_src == s->x_dst || s->c_src == s->c_dst || s->w_src == s->w_dst) return ASR_E_ARG;   // a gather: out of place
  return 0;
}

// the checks of an asr_beam_*_tlm call (before any launch), and the device's view of its LM and extra workspace
int tlm_args(const asr_beam_t* p, const asr_beam_tlm_t* lm, bool need_logits, BeamTlm<true>* g) {
  int rc = check_beam(p, need_logits);
  if (rc) return rc;
  if (!lm || !lm->ws || !(fabsf(lm->weight) <= FLT_MAX) || !(fabsf(lm->bonus) <= FLT_MAX)) return ASR_E_ARG;
  if (lm->ws_bytes < tlm_ws_bytes(p->B, p->K) || (((uintptr_t)lm->ws) & 3u)) return ASR_E_ARG;
  *g = BeamTlm<true>{};
  if (lm->kind == ASR_BEAM_TLM_NGRAM) {
    if (!lm->lm_logp || !lm->lm_next || lm->lm_states <= 0) return ASR_E_ARG;
    if ((int64_t)lm->lm_states * p->V > INT_MAX || lm->lm_start < 0 || lm->lm_start >= lm->lm_states) return ASR_E_SHAPE;
    g->logp = lm->lm_logp, g->next = lm->lm_next, g->start = lm->lm_start;
  } else if (lm->kind == ASR_BEAM_TLM_WORD) {
    rc = wlm::check_abi(lm->word_lm);
    if (rc) return rc;
    if (lm->word_lm->V != p->V) return ASR_E_SHAPE;
    g->w = wlm::from_abi(*lm->word_lm);
  } else {
    return ASR_E_ARG;
  }
  g->weight = lm->weight, g->bonus = lm->bonus;
  g->lexicon_only = lm->kind == ASR_BEAM_TLM_WORD && lm->lexicon_only != 0;
  const int64_t n_bk = round64((int64_t)p->B * p->K), n_f = round64((int64_t)p->B * BEAM_FCAP);
  g->a = (int32_t*)lm->ws;
  g->b = g->a + n_bk;
  g->n = g->b + n_bk;
  g->lm = (float*)(g->n + n_bk);
  g->fin_base = g->lm + n_bk;
  g->fin_lm = g->fin_base + n_f;
  g->fin_n = (int32_t*)(g->fin_lm + n_f);
  return 0;
}

}  // namespace

extern "C" int asr_beam_select_f32(const asr_beam_t* p, int t, asr_stream_t stream_) {
  const int rc = check_step(p, t);
  return rc ? rc : beam_select(p, t, nullptr, 0.f, nullptr, nullptr, 0.f, TLM_NONE, nullptr, (hipStream_t)stream_);
}

extern "C" int asr_beam_select_lm_f32(const asr_beam_t* p, const float* lm_logits, float lm_weight, int t,
                                      asr_stream_t stream_) {
  if (!lm_logits) return ASR_E_ARG;
  const int rc = check_step(p, t);
  return rc ? rc : beam_select(p, t, lm_logits, lm_weight, nullptr, nullptr, 0.f, TLM_NONE, nullptr, (hipStream_t)stream_);
}

extern "C" int asr_beam_select_ctc_f32(const asr_beam_t* p, const float* lm_logits, float lm_weight, const float* psi,
                                       const float* psi_prev, float ctc_weight, int t, asr_stream_t stream_) {
  int rc = check_ctc(p, psi, psi_prev, ctc_weight);
  if (!rc) rc = check_step(p, t);
  return rc ? rc : beam_select(p, t, lm_logits, lm_weight, psi, psi_prev, ctc_weight, TLM_NONE, nullptr, (hipStream_t)stream_);
}

extern "C" int asr_beam_reorder_f32(const asr_beam_t* p, int t, const asr_beam_state_t* s, asr_stream_t stream_) {
  int rc = check_beam(p, false);
  if (rc) return rc;
  rc = check_beam_state(p, t, s);
  if (rc) return rc;
  hipLaunchKernelGGL(beam_reorder_kernel, dim3(p->B * p->K), dim3(BEAM_NT), 0, (hipStream_t)stream_, *p, t, *s);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_beam_reorder_lm_f32(const asr_beam_t* p, int t, const asr_beam_state_t* s, const asr_beam_lm_state_t* m,
                                       asr_stream_t stream_) {
  int rc = check_beam(p, false);
  if (rc) return rc;
  if (!m || !m->emb || t < 0 || t >= p->L) return ASR_E_ARG;
  if (s && (rc = check_beam_state(p, t, s))) return rc;
  if (m->n_layers < 1 || m->n_layers > ASR_LM_MAX_LAYERS || m->H <= 0) return ASR_E_SHAPE;
  for (int l = 0; l < m->n_layers; ++l) {
    if (!m->x_src[l] || !m->x_dst[l] || !m->c_src[l] || !m->c_dst[l] || m->in_dim[l] <= 0) return ASR_E_ARG;
    if (m->x_src[l] == m->x_dst[l] || m->c_src[l] == m->c_dst[l]) return ASR_E_ARG;            // a gather: out of place
  }
  asr_beam_state_t none = {};
  hipLaunchKernelGGL(beam_reorder_lm_kernel, dim3(p->B * p->K, 1 + m->n_layers), dim3(BEAM_NT), 0, (hipStream_t)stream_, *p,
                     t, s ? *s : none, s ? 1 : 0, *m);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_beam_backtrack(const asr_beam_t* p, float length_penalty, int32_t* tokens, float* scores,
                                  int32_t* lengths, asr_stream_t stream_) {
  int rc = check_beam(p, false);
  if (rc) return rc;
  if (!tokens || !scores || !lengths) return ASR_E_ARG;
  hipLaunchKernelGGL(beam_backtrack_kernel<false>, dim3(p->B), dim3(BEAM_NT), 0, (hipStream_t)stream_, *p, length_penalty,
                     tokens, scores, lengths, beam_parts_args<false>());
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_beam_tlm_ws_bytes(int B, int K, int64_t* ws_bytes) {
  if (!ws_bytes || B <= 0) return ASR_E_ARG;
  if (K < 1 || K > BEAM_KMAX) return ASR_E_SHAPE;
  *ws_bytes = tlm_ws_bytes(B, K);
  return 0;
}

extern "C" int asr_beam_tlm_init_f32(const asr_beam_t* p, const asr_beam_tlm_t* lm, asr_stream_t stream_) {
  BeamTlm<true> g;
  const int rc = tlm_args(p, lm, false, &g);
  if (rc) return rc;
  const int R = p->B * p->K;
  const dim3 grid((R + BEAM_NT - 1) / BEAM_NT), block(BEAM_NT);
  if (lm->kind == ASR_BEAM_TLM_NGRAM) hipLaunchKernelGGL(beam_tlm_init_kernel<TLM_NGRAM>, grid, block, 0, (hipStream_t)stream_, R, g);
  else hipLaunchKernelGGL(beam_tlm_init_kernel<TLM_WORD>, grid, block, 0, (hipStream_t)stream_, R, g);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_beam_select_tlm_f32(const asr_beam_t* p, const asr_beam_tlm_t* lm, const float* lm_logits, float lm_weight,
                                       const float* psi, const float* psi_prev, float ctc_weight, int t, asr_stream_t stream_) {
  BeamTlm<true> g;
  int rc = tlm_args(p, lm, true, &g);
  if (!rc) rc = check_step(p, t);
  if (!rc) rc = check_ctc(p, psi, psi_prev, ctc_weight);
  if (rc) return rc;
  return beam_select(p, t, lm_logits, lm_weight, psi, psi_prev, ctc_weight, lm->kind == ASR_BEAM_TLM_WORD ? TLM_WORD : TLM_NGRAM,
                     &g, (hipStream_t)stream_);
}

extern "C" int asr_beam_backtrack_tlm(const asr_beam_t* p, const asr_beam_tlm_t* lm, float length_penalty, int32_t* tokens,
                                      float* scores, int32_t* lengths, float* att_score, float* lm_score, int32_t* n_out,
                                      asr_stream_t stream_) {
  BeamTlm<true> g;
  const int rc = tlm_args(p, lm, false, &g);
  if (rc) return rc;
  if (!tokens || !scores || !lengths || !att_score || !lm_score || !n_out) return ASR_E_ARG;
  beam_parts_args<true> pa;
  pa.fin_base = g.fin_base, pa.fin_lm = g.fin_lm, pa.fin_n = g.fin_n;
  pa.out_base = att_score, pa.out_lm = lm_score, pa.out_n = n_out;
  hipLaunchKernelGGL(beam_backtrack_kernel<true>, dim3(p->B), dim3(BEAM_NT), 0, (hipStream_t)stream_, *p, length_penalty,
                     tokens, scores, lengths, pa);
  ASR_CHECK_LAUNCH();
  return 0;
}
