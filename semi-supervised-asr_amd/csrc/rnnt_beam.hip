// rnnt_beam.hip — beam search over the transducer head, with an n-gram LM inside when one is given.  The
// conventions are seq_common.h's (blank = 0, candidates rank by `better`, ordered sums, no floating-point atomics); the
// head is rnnt.hip's.  The search is alignment-length synchronous: at iteration i every entry of an utterance's beam sits
// on the anti-diagonal t + u = i of the lattice (u: its label count, t = i - u: its frame), every entry moves one step per
// iteration - the blank to (t + 1, u), a label to (t, u + 1) - and a fixed T + L iterations finish every row: no host read.
// Two candidates that are the same label sequence at the same node - the blank candidate of entry h and the label candidate
// (h', k) with seq(h') . k = seq(h) - are ONE candidate whose mass is the logaddexp of the two: the lattice recursion
// alpha(t, u) of the loss, restricted to the beam.  Equal sequences are found as ctc_beam.hip finds them, by
// seq_common.h's merge identity (prefix_hash and the length), and ranks are its lm_rank.  The merged candidate keeps the flat index, the
// prediction-network state and the history record of its BLANK parent: its bits are a function of the inputs.
//   rnnt_beam_init_kernel       the empty sequence at (0, 0) in slot 0 of every utterance with a frame, the gathered cell
//                               input [emb(<BOS>) | 0] with advance = 1 for it, zeros for the other slots
//   rnnt_beam_step_kernel       one workgroup per utterance, one iteration: tanh of the live entries into LDS [K][J]; the
//                               J x V products, a wave per (entry, vocabulary item), lanes strided over J, the xor butterfly
//                               (the greedy kernel's arithmetic); the row log-sum-exp (wave_row_max_sumexp); the blank
//                               candidates with their merge partner's mass; the candidate walk (entry-major, tokens strided
//                               over the threads: ascending flat index parent V + token) into sorted register lists
//                               (top_insert); K rounds of the workgroup arg-best (top_round); then the new beam, a history
//                               record (token, parent slot) per slot, the `advance` flags, and the cell's gathered input
//                               [emb(token) | h(parent)], c(parent).  A blank taken at t = T_b - 1 is a FINAL: it leaves
//                               the beam for the utterance's final list (iteration, slot, u, tot, lm, rank; the best K by
//                               rank, the earlier one first on ties).  A sequence finalises at most once - a sequence of u
//                               labels can do so only at iteration T_b - 1 + u, and a beam holds a sequence once - so finals
//                               never need merging.
//   rnnt_beam_cell_kernel       the pointwise half of the prediction cell: h', c' from the gate product where `advance` is
//                               set, the parent's h, c (as gathered) elsewhere
//   rnnt_beam_backtrace_kernel  one thread per final: the history walked back into hyp
// Frames t >= T_b, slots that are not live and workspace words that this call has not written are never read.
// LDS of the step kernel: K (J + V) floats (dynamic) and under 2 KB of per-entry arrays: K (J + V) * 4 <= kBeamLds.
// With a word LM and its lexicon inside the search (the kernels' WLM instantiations, the asr_transducer_wbeam_*
// entries) an entry additionally carries its trie node, its word state, lm - the sum over its COMPLETED words - and their
// count nw: functions of the token sequence, so the merge and prefix identity are untouched.  One thread per live entry
// does the entry's lookups (word_lm.h's close_pair, which is what a `space` candidate and a final both need, and its finish
// for a final) into LDS; the new beam moves by its after_token; the candidate walk reads them, and with lexicon_only one
// trie_next word per (entry, token).  The instantiations without it hold none of this.
#include <float.h>
#include <type_traits>
#include "seq_common.h"
#include "word_lm.h"

namespace {

constexpr int kKmax = ASR_BEAM_KMAX;
constexpr int kThreads = 256;
constexpr int kBeamLds = ASR_RNNT_BEAM_LDS_BYTES;
static_assert(kKmax <= 32, "the merge map of an entry is one 32-bit mask");
static_assert(kBeamLds + 4096 <= 64 * 1024, "dynamic and static LDS of the step kernel inside 64 KB");

struct BeamWs {
  u64* hash;           // [2][B K]
  int2* hist;          // [T + L][B][K] (token, parent slot); token 0: the blank
  float* tot;          // [2][B K]
  float* lm;           // [2][B K]
  int32_t* state;      // [2][B K]   the LM automaton's state
  int32_t* u;          // [2][B K]   labels of the entry
  int32_t* last;       // [2][B K]   its last label (-1: none)
  int32_t* nlive;      // [2][B]
  int32_t* advance;    // [B K]
  float* cg;           // [B K][P]   c of the parent slot
  int32_t* fin_it;     // [B K]      the finals, ranked
  int32_t* fin_slot;
  int32_t* fin_u;
  float* fin_tot;
  float* fin_lm;
  float* fin_rank;
  int32_t* nfin;       // [B]
  int64_t bytes;
};

BeamWs beam_ws(void* base, int B, int T, int K, int L, int P) {
  const int64_t n_bk = round64((int64_t)B * K), n_b = round64(B), n_h = round64((int64_t)(T + L) * B * K);
  const int64_t n_c = round64((int64_t)B * K * P);
  BeamWs w;
  w.hash = (u64*)base;                                       // (the 8-byte regions first)
  w.hist = (int2*)(w.hash + 2 * n_bk);
  w.tot = (float*)(w.hist + n_h);
  w.lm = w.tot + 2 * n_bk;
  w.state = (int32_t*)(w.lm + 2 * n_bk);
  w.u = w.state + 2 * n_bk;
  w.last = w.u + 2 * n_bk;
  w.nlive = w.last + 2 * n_bk;
  w.advance = w.nlive + 2 * n_b;
  w.cg = (float*)(w.advance + n_bk);
  w.fin_it = (int32_t*)(w.cg + n_c);
  w.fin_slot = w.fin_it + n_bk;
  w.fin_u = w.fin_slot + n_bk;
  w.fin_tot = (float*)(w.fin_u + n_bk);
  w.fin_lm = w.fin_tot + n_bk;
  w.fin_rank = w.fin_lm + n_bk;
  w.nfin = (int32_t*)(w.fin_rank + n_bk);
  w.bytes = 8 * (2 * n_bk + n_h) + 4 * (10 * n_bk + 2 * n_b + n_bk + n_c + 6 * n_bk + n_b);
  return w;
}

// the word LM of a fused search and the entries' word state: the EXTRA workspace of the asr_transducer_wbeam_* entries
struct BeamWlm {
  wlm::WordLm w;
  int N, S;                // trie nodes, word states: what is read back from the workspace is clamped to them
  float alpha, beta;
  int eos_term, lexicon_only;
  int32_t* node;           // [2][B K]   the trie node of the entry's pending word (0: the root, -1: off the trie)
  int32_t* wst;            // [2][B K]   its word-LM state
  int32_t* nw;             // [2][B K]   its completed words
  int32_t* fin_nw;         // [B K]      the finals' words
};
struct NoWlm {};

int64_t wbeam_ws_bytes(int B, int K) { return 4 * 7 * round64((int64_t)B * K); }

int beam_shape_check(int B, int T, int J, int V, int K, int L, int E, int P) {
  if (B <= 0 || T <= 0 || J <= 0 || V <= 0 || L <= 0 || E <= 0 || P <= 0) return ASR_E_ARG;
  if (K < 1 || K > kKmax || V < 2 || (J & 3) || (int64_t)K * ((int64_t)J + V) * 4 > kBeamLds) return ASR_E_SHAPE;
  if ((int64_t)K * V > INT_MAX / 2 || (int64_t)B * K * ((int64_t)E + 4 * (int64_t)P) > INT_MAX ||
      ((int64_t)T + L) * B * K > INT_MAX)
    return ASR_E_SHAPE;
  return 0;
}

template <bool WLM>
__global__ __launch_bounds__(kThreads) void rnnt_beam_init_kernel(asr_transducer_beam_t a, int bos, BeamWs w,
                                                                  std::conditional_t<WLM, BeamWlm, NoWlm> g) {
  const int b = blockIdx.x, tid = threadIdx.x, K = a.K, EP = a.E + a.P;
  const int live = clamp_len(a.frame_lens[b], a.T) > 0 ? 1 : 0;
  if (tid == 0) {
    w.nlive[b] = live;
    w.nfin[b] = 0;
    if (live) {
      const int64_t s = (int64_t)b * K;
      w.tot[s] = 0.f;
      w.lm[s] = 0.f;
      w.state[s] = a.lm_logp ? a.lm_start : 0;
      w.u[s] = 0;
      w.last[s] = -1;
      w.hash[s] = 0;
      if constexpr (WLM) {
        g.node[s] = 0;
        g.wst[s] = g.w.start;
        g.nw[s] = 0;
      }
    }
  }
  if (tid < K) w.advance[(int64_t)b * K + tid] = (tid == 0 && live) ? 1 : 0;
  float* xh = a.xh + (int64_t)b * K * EP;
  for (int i = tid; i < K * EP; i += kThreads) xh[i] = (live && i < a.E) ? a.emb[(int64_t)bos * a.E + i] : 0.f;
  float* cg = w.cg + (int64_t)b * K * a.P;
  for (int i = tid; i < K * a.P; i += kThreads) cg[i] = 0.f;
}

template <bool WLM>
__global__ __launch_bounds__(kThreads) void rnnt_beam_step_kernel(asr_transducer_beam_t a, int it, BeamWs w,
                                                                  std::conditional_t<WLM, BeamWlm, NoWlm> g) {
  extern __shared__ float sm[];
  __shared__ float s_tot[kKmax], s_lm[kKmax], s_lse[kKmax], s_btot[kKmax];
  __shared__ int s_u[kKmax], s_last[kKmax], s_state[kKmax], s_fin[kKmax], s_par[kKmax], s_tok[kKmax];
  __shared__ u64 s_hash[kKmax];
  __shared__ unsigned s_mk[kKmax];                           // entry h': the entries that are seq(h') + one label
  // (word LM only: unused arrays take no LDS) the entry's node, word state and words; the close pair of its pending word
  // (next < 0: lexicon_only and the node ends no word); lm, words and admission of the entry as a final
  __shared__ int s_node[kKmax], s_wst[kKmax], s_nw[kKmax], s_snx[kKmax], s_fnw[kKmax], s_fok[kKmax];
  __shared__ float s_slp[kKmax], s_flm[kKmax];
  __shared__ float red_v[2][kThreads / 64];
  __shared__ int red_i[2][kThreads / 64];
  const int B = a.B, T = a.T, J = a.J, V = a.V, K = a.K, L = a.L, E = a.E, P = a.P, EP = a.E + a.P;
  float* zj = sm;                                            // [K][J]
  float* lg = sm + (int64_t)K * J;                           // [K][V]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = kThreads >> 6;
  const int64_t bk = (int64_t)B * K, src = (int64_t)(it & 1) * bk + (int64_t)b * K, dst = (int64_t)((it & 1) ^ 1) * bk + (int64_t)b * K;
  const int len = clamp_len(a.frame_lens[b], T);
  int nlive = w.nlive[(int64_t)(it & 1) * B + b];
  nlive = nlive < 0 ? 0 : (nlive > K ? K : nlive);
  const bool lmode = !WLM && a.lm_logp != nullptr;
  float* xh = a.xh + (int64_t)b * K * EP;
  float* cg = w.cg + (int64_t)b * K * P;
  if (nlive == 0) {                                          // every hypothesis of the row has finalised (or it has no frame)
    if (tid == 0) w.nlive[(int64_t)((it & 1) ^ 1) * B + b] = 0;
    if (tid < K) w.advance[(int64_t)b * K + tid] = 0;
    for (int i = tid; i < K * EP; i += kThreads) xh[i] = 0.f;
    for (int i = tid; i < K * P; i += kThreads) cg[i] = 0.f;
    return;
  }
  if (tid < nlive) {
    s_tot[tid] = w.tot[src + tid];
    s_lm[tid] = w.lm[src + tid];
    s_u[tid] = w.u[src + tid];
    s_last[tid] = w.last[src + tid];
    s_state[tid] = w.state[src + tid];
    s_hash[tid] = w.hash[src + tid];
    if constexpr (WLM) {                                     // (what indexes the tables is clamped)
      const int nd = g.node[src + tid], st = g.wst[src + tid];
      s_node[tid] = nd < 0 ? -1 : (nd >= g.N ? g.N - 1 : nd);
      s_wst[tid] = st < 0 ? 0 : (st >= g.S ? g.S - 1 : st);
      s_nw[tid] = g.nw[src + tid];
    }
  }
  __syncthreads();
  // Z = tanh(PE[b][t_h] + PP[h]); t_h = it - u_h lies in [0, T_b) for a live entry (clamped for the address all the same)
  for (int i = tid; i < nlive * J; i += kThreads) {
    const int h = i / J, j = i - h * J;
    int t = it - s_u[h];
    t = t < 0 ? 0 : (t >= len ? len - 1 : t);
    zj[i] = tanhf(a.pe[((int64_t)b * T + t) * J + j] + a.pp[((int64_t)b * K + h) * J + j]);
  }
  __syncthreads();
  for (int pr = wave; pr < nlive * V; pr += nw) {
    const int h = pr / V, k = pr - h * V;
    const float* wr = a.w_out + (int64_t)k * J;
    const float* zr = zj + (int64_t)h * J;
    float s = 0.f;
    for (int j = lane; j < J; j += 64) s += zr[j] * wr[j];
    s = wave_sum(s);
    if (lane == 0) lg[pr] = s + (a.b_out ? a.b_out[k] : 0.f);
  }
  __syncthreads();
  for (int h = wave; h < nlive; h += nw) {
    float mx, se;
    wave_row_max_sumexp(lg + (int64_t)h * V, V, lane, mx, se);
    if (lane == 0) s_lse[h] = mx + logf(se);
  }
  __syncthreads();
  // the blank candidate of entry tid with the mass of its merge partner, and the merge map of entry tid
  if (tid < nlive) {
    const int uh = s_u[tid], ch = s_last[tid];
    const u64 hh = s_hash[tid];
    const int fin = (it - uh) >= len - 1 ? 1 : 0;
    float bt = s_tot[tid] + (lg[tid * V] - s_lse[tid]);
    unsigned mk = 0;
    for (int i = 0; i < nlive; ++i) {
      // seq(i) . ch is this entry: the label candidate (i, ch) lands on this entry's blank node (never a final: entry i
      // sits one frame later than this one)
      if (!fin && ch > 0 && s_u[i] + 1 == uh && prefix_hash(s_hash[i], ch) == hh)
        bt = logaddexp(bt, s_tot[i] + (lg[i * V + ch] - s_lse[i]));
      if (s_u[i] == uh + 1 && s_last[i] > 0 && prefix_hash(hh, s_last[i]) == s_hash[i]) mk |= 1u << i;
    }
    s_btot[tid] = bt;
    s_fin[tid] = fin;
    s_mk[tid] = mk;
    if constexpr (WLM) {
      // the close pair of the pending word: what a `space` candidate of this entry, and this entry as a final, add
      wlm::WordPos e{s_node[tid], s_wst[tid], s_lm[tid], s_nw[tid]};
      float lp;
      int nx;
      wlm::close_pair(g.w, e.node, e.state, g.lexicon_only != 0, lp, nx);
      s_slp[tid] = lp;
      s_snx[tid] = nx;
      if (fin) {
        s_fok[tid] = wlm::finish(g.w, e, lp, nx, g.eos_term != 0) ? 1 : 0;
        s_flm[tid] = e.lm;
        s_fnw[tid] = e.nw;
      }
    }
  }
  __syncthreads();
  // the candidates, entry-major: a thread meets its flat indices h V + k in ascending order
  float lv[kKmax];
  int li[kKmax];
  top_clear(lv, li);
  for (int h = 0; h < nlive; ++h) {
    const int uh = s_u[h];
    const float toth = s_tot[h], lseh = s_lse[h], lmh = s_lm[h];
    const unsigned mkh = s_mk[h];
    const float* lrow = lmode ? a.lm_logp + (int64_t)s_state[h] * V : nullptr;
    for (int k = tid; k < V; k += kThreads) {
      float val, lmv = lmh;
      int uv = uh;
      if (k == 0) {
        val = s_fin[h] ? -INFINITY : s_btot[h];
        if constexpr (WLM) uv = s_nw[h];
      } else {
        if (uh >= L) continue;
        if constexpr (WLM) {                                 // (uv: the candidate's completed words)
          const int nd = s_node[h];
          uv = s_nw[h];
          if (k == g.w.space) {
            if (nd != 0) {
              if (s_snx[h] < 0) continue;
              lmv = __fadd_rn(lmh, s_slp[h]);
              ++uv;
            }
          } else if (g.lexicon_only && wlm::trie_step(g.w, nd, k) < 0) {
            continue;
          }
        }
        val = toth + (lg[h * V + k] - lseh);
        for (unsigned m = mkh; m; m &= m - 1)                // seq(h) . k is in the beam: it joins that entry's blank
          if (s_last[__ffs(m) - 1] == k) val = -INFINITY;
        if (lmode) lmv = lmh + lrow[k];
        if constexpr (!WLM) uv = uh + 1;
      }
      if constexpr (WLM) top_insert(lv, li, lm_rank(val, lmv, uv, g.alpha, g.beta), h * V + k);
      else top_insert(lv, li, lmode ? lm_rank(val, lmv, uv, a.lm_alpha, a.lm_beta) : val, h * V + k);
    }
  }
  int nsel = 0, my_i = INT_MAX;
  for (int r = 0; r < K; ++r) {
    float bv;
    int bi;
    top_round(lv[0], li[0], red_v[r & 1], red_i[r & 1], nw, bv, bi);
    if (!(bv > -INFINITY)) break;                            // (the same in every thread)
    top_pop_if_head(lv, li, bi);
    if (tid == r) my_i = bi;
    ++nsel;
  }
  // the new beam; slot r holds the r-th best
  if (tid < K) {
    int adv = 0;
    if (tid < nsel) {
      const int h = my_i / V, k = my_i - h * V;
      const int64_t d = dst + tid;
      if (k == 0) {
        w.tot[d] = s_btot[h];
        w.lm[d] = s_lm[h];
        w.state[d] = s_state[h];
        w.u[d] = s_u[h];
        w.last[d] = s_last[h];
        w.hash[d] = s_hash[h];
      } else {
        w.tot[d] = s_tot[h] + (lg[h * V + k] - s_lse[h]);
        w.lm[d] = lmode ? s_lm[h] + a.lm_logp[(int64_t)s_state[h] * V + k] : 0.f;
        w.state[d] = lmode ? a.lm_next[(int64_t)s_state[h] * V + k] : 0;
        w.u[d] = s_u[h] + 1;
        w.last[d] = k;
        w.hash[d] = prefix_hash(s_hash[h], k);
        adv = 1;
      }
      if constexpr (WLM) {
        wlm::WordPos e{s_node[h], s_wst[h], s_lm[h], s_nw[h]};
        if (k != 0) e = wlm::after_token(g.w, e, k, s_slp[h], s_snx[h]);
        w.lm[d] = e.lm;
        g.node[d] = e.node;
        g.wst[d] = e.state;
        g.nw[d] = e.nw;
      }
      w.hist[((int64_t)it * B + b) * K + tid] = make_int2(k, h);
      s_par[tid] = h;
      s_tok[tid] = k;
    }
    w.advance[(int64_t)b * K + tid] = adv;
  }
  if (tid == 0) {
    w.nlive[(int64_t)((it & 1) ^ 1) * B + b] = nsel;
    // the finals of this iteration, in slot order, into the ranked list: a final displaces only strictly worse ones
    int n = w.nfin[b];
    n = n < 0 ? 0 : (n > K ? K : n);
    const int64_t f0 = (int64_t)b * K;
    for (int h = 0; h < nlive; ++h) {
      if (!s_fin[h]) continue;
      const float ft = s_btot[h];
      float fl = s_lm[h], fr;
      if constexpr (WLM) {
        if (!s_fok[h]) continue;                             // lexicon_only: the pending node ends no word
        fl = s_flm[h];
        fr = lm_rank(ft, fl, s_fnw[h], g.alpha, g.beta);
      } else {
        if (lmode && a.lm_eos >= 0) fl = fl + a.lm_logp[(int64_t)s_state[h] * V + a.lm_eos];
        fr = lmode ? lm_rank(ft, fl, s_u[h], a.lm_alpha, a.lm_beta) : ft;
      }
      if (!(fr > -INFINITY)) continue;
      int p = 0;
      while (p < n && w.fin_rank[f0 + p] >= fr) ++p;
      if (p >= K) continue;
      const int last = n < K ? n : K - 1;
      for (int q = last; q > p; --q) {
        w.fin_it[f0 + q] = w.fin_it[f0 + q - 1];
        w.fin_slot[f0 + q] = w.fin_slot[f0 + q - 1];
        w.fin_u[f0 + q] = w.fin_u[f0 + q - 1];
        w.fin_tot[f0 + q] = w.fin_tot[f0 + q - 1];
        w.fin_lm[f0 + q] = w.fin_lm[f0 + q - 1];
        w.fin_rank[f0 + q] = w.fin_rank[f0 + q - 1];
        if constexpr (WLM) g.fin_nw[f0 + q] = g.fin_nw[f0 + q - 1];
      }
      w.fin_it[f0 + p] = it;
      w.fin_slot[f0 + p] = h;
      w.fin_u[f0 + p] = s_u[h];
      w.fin_tot[f0 + p] = ft;
      w.fin_lm[f0 + p] = fl;
      w.fin_rank[f0 + p] = fr;
      if constexpr (WLM) g.fin_nw[f0 + p] = s_fnw[h];
      if (n < K) ++n;
    }
    w.nfin[b] = n;
  }
  __syncthreads();
  // the cell's input of every slot: [emb(token) | h(parent)] and c(parent); zeros in slots that are not live
  for (int i = tid; i < K * EP; i += kThreads) {
    const int s = i / EP, col = i - s * EP;
    float v = 0.f;
    if (s < nsel) {
      if (col >= E) v = a.h[((int64_t)b * K + s_par[s]) * P + (col - E)];
      else if (s_tok[s] > 0) v = a.emb[(int64_t)s_tok[s] * E + col];
    }
    xh[i] = v;
  }
  for (int i = tid; i < K * P; i += kThreads) {
    const int s = i / P, col = i - s * P;
    cg[i] = s < nsel ? a.c[((int64_t)b * K + s_par[s]) * P + col] : 0.f;
  }
}

// gates [B K][4 P] in torch's order i, f, g, o
__global__ __launch_bounds__(256) void rnnt_beam_cell_kernel(int64_t total, int E, int P, const float* __restrict__ gates,
                                                             const float* __restrict__ xh, const float* __restrict__ cg,
                                                             const int32_t* __restrict__ advance, float* __restrict__ h,
                                                             float* __restrict__ c) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t row = idx / P;
  const int p = (int)(idx - row * P);
  float c2 = cg[idx], h2 = xh[row * (E + P) + E + p];
  if (advance[row]) {
    const float* g = gates + row * 4 * P;
    c2 = asr_sigmoid(g[P + p]) * c2 + asr_sigmoid(g[p]) * tanhf(g[2 * P + p]);
    h2 = asr_sigmoid(g[3 * P + p]) * tanhf(c2);
  }
  h[idx] = h2;
  c[idx] = c2;
}

template <bool WLM>
__global__ __launch_bounds__(64) void rnnt_beam_backtrace_kernel(asr_transducer_beam_t a, BeamWs w, int32_t* __restrict__ hyp,
                                                                 int32_t* __restrict__ hyp_len, float* __restrict__ score,
                                                                 float* __restrict__ rnnt_score, float* __restrict__ lm_score,
                                                                 std::conditional_t<WLM, BeamWlm, NoWlm> g,
                                                                 int32_t* __restrict__ n_words) {
  const int b = blockIdx.x, r = threadIdx.x, B = a.B, K = a.K, L = a.L;
  if (r >= K) return;
  const int64_t o = (int64_t)b * K + r;
  int32_t* hr = hyp + o * L;
  const int len = clamp_len(a.frame_lens[b], a.T);
  const bool lmode = !WLM && a.lm_logp != nullptr;
  int n = 0, u = -1, words = -1;
  float tot = -INFINITY, lm = -INFINITY, rank = -INFINITY;
  if (len == 0) {                                            // no frames: the empty hypothesis at score 0, nothing else
    if (r == 0) {
      u = 0;
      tot = 0.f;
      if constexpr (WLM) {
        wlm::WordPos e = wlm::start_pos(g.w);
        wlm::finish(g.w, e, 0.f, e.state, g.eos_term != 0);
        lm = e.lm;
        words = 0;
        rank = lm_rank(0.f, lm, 0, g.alpha, g.beta);
      } else {
        lm = (lmode && a.lm_eos >= 0) ? a.lm_logp[(int64_t)a.lm_start * a.V + a.lm_eos] : 0.f;
        rank = lmode ? lm_rank(0.f, lm, 0, a.lm_alpha, a.lm_beta) : 0.f;
      }
    }
  } else {
    n = w.nfin[b];
    n = n < 0 ? 0 : (n > K ? K : n);
    if (r < n) {
      u = w.fin_u[o];
      u = u < 0 ? 0 : (u > L ? L : u);
      tot = w.fin_tot[o];
      lm = w.fin_lm[o];
      rank = w.fin_rank[o];
      if constexpr (WLM) words = g.fin_nw[o];
      int s = w.fin_slot[o] & (kKmax - 1), pos = u - 1;
      for (int j = w.fin_it[o] - 1; j >= 0 && pos >= 0; --j) {
        const int2 rec = w.hist[((int64_t)j * B + b) * K + s];
        if (rec.x > 0) hr[pos--] = rec.x;
        s = rec.y & (kKmax - 1);
      }
      for (; pos >= 0; --pos) hr[pos] = -1;                  // (not reached: u labels lie on the way back)
    }
  }
  for (int i = u < 0 ? 0 : u; i < L; ++i) hr[i] = -1;
  hyp_len[o] = u;
  score[o] = rank;
  if (rnnt_score) rnnt_score[o] = tot;
  if (lm_score) lm_score[o] = lm;
  if constexpr (WLM) n_words[o] = words;
}

int beam_args_check(const asr_transducer_beam_t* a) {
  if (!a) return ASR_E_ARG;
  const int rc = beam_shape_check(a->B, a->T, a->J, a->V, a->K, a->L, a->E, a->P);
  if (rc) return rc;
  if (!a->pe || !a->pp || !a->w_out || !a->emb || !a->frame_lens || !a->h || !a->c || !a->xh || !a->ws) return ASR_E_ARG;
  if (a->lm_logp && (!a->lm_next || a->lm_states <= 0)) return ASR_E_ARG;
  if (a->lm_logp && (a->lm_start < 0 || a->lm_start >= a->lm_states || a->lm_eos >= a->V)) return ASR_E_SHAPE;
  if (a->ws_bytes < beam_ws(nullptr, a->B, a->T, a->K, a->L, a->P).bytes || (((uintptr_t)a->ws) & 7u)) return ASR_E_ARG;
  return 0;
}

// the checks of an asr_transducer_wbeam_* call, and the device's view of its LM and extra workspace
int wbeam_args(const asr_transducer_beam_t* a, const asr_word_lm_t* lm, float alpha, float beta, int eos_term, int lexicon_only,
               void* wws, int64_t wws_bytes, BeamWlm* g) {
  int rc = beam_args_check(a);
  if (rc) return rc;
  if (a->lm_logp || !wws || !(fabsf(alpha) <= FLT_MAX) || !(fabsf(beta) <= FLT_MAX)) return ASR_E_ARG;
  rc = wlm::check_abi(lm);
  if (rc) return rc;
  if (lm->V != a->V) return ASR_E_SHAPE;
  if (wws_bytes < wbeam_ws_bytes(a->B, a->K) || (((uintptr_t)wws) & 3u)) return ASR_E_ARG;
  const int64_t n_bk = round64((int64_t)a->B * a->K);
  g->w = wlm::from_abi(*lm);
  g->N = lm->N, g->S = lm->S;
  g->alpha = alpha, g->beta = beta, g->eos_term = eos_term != 0, g->lexicon_only = lexicon_only != 0;
  g->node = (int32_t*)wws;
  g->wst = g->node + 2 * n_bk;
  g->nw = g->wst + 2 * n_bk;
  g->fin_nw = g->nw + 2 * n_bk;
  return 0;
}

// The launches behind both entry families (g: NoWlm() or the BeamWlm of wbeam_args); `a` has passed the entry's checks.
template <bool WLM>
int launch_init(const asr_transducer_beam_t* a, int bos, const std::conditional_t<WLM, BeamWlm, NoWlm>& g, asr_stream_t stream) {
  if (bos < 0 || bos >= a->V) return ASR_E_ARG;
  hipLaunchKernelGGL(rnnt_beam_init_kernel<WLM>, dim3(a->B), dim3(kThreads), 0, (hipStream_t)stream, *a, bos,
                     beam_ws(a->ws, a->B, a->T, a->K, a->L, a->P), g);
  ASR_CHECK_LAUNCH();
  return 0;
}

template <bool WLM>
int launch_step(const asr_transducer_beam_t* a, int it, const std::conditional_t<WLM, BeamWlm, NoWlm>& g, asr_stream_t stream) {
  if (it < 0 || it >= a->T + a->L) return ASR_E_ARG;
  hipLaunchKernelGGL(rnnt_beam_step_kernel<WLM>, dim3(a->B), dim3(kThreads), (size_t)a->K * ((size_t)a->J + a->V) * 4,
                     (hipStream_t)stream, *a, it, beam_ws(a->ws, a->B, a->T, a->K, a->L, a->P), g);
  ASR_CHECK_LAUNCH();
  return 0;
}

template <bool WLM>
int launch_backtrace(const asr_transducer_beam_t* a, int32_t* hyp, int32_t* hyp_len, float* score, float* rnnt_score,
                     float* lm_score, const std::conditional_t<WLM, BeamWlm, NoWlm>& g, int32_t* n_words, asr_stream_t stream) {
  if (!hyp || !hyp_len || !score || (WLM && !n_words)) return ASR_E_ARG;
  hipLaunchKernelGGL(rnnt_beam_backtrace_kernel<WLM>, dim3(a->B), dim3(64), 0, (hipStream_t)stream, *a,
                     beam_ws(a->ws, a->B, a->T, a->K, a->L, a->P), hyp, hyp_len, score, rnnt_score, lm_score, g, n_words);
  ASR_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int asr_transducer_beam_ws_bytes(int B, int T, int J, int V, int K, int L, int E, int P, int64_t* ws_bytes) {
  if (!ws_bytes) return ASR_E_ARG;
  const int rc = beam_shape_check(B, T, J, V, K, L, E, P);
  if (rc) return rc;
  *ws_bytes = beam_ws(nullptr, B, T, K, L, P).bytes;
  return 0;
}

extern "C" int asr_transducer_beam_init_f32(const asr_transducer_beam_t* a, int bos, asr_stream_t stream) {
  const int rc = beam_args_check(a);
  return rc ? rc : launch_init<false>(a, bos, NoWlm(), stream);
}

extern "C" int asr_transducer_beam_step_f32(const asr_transducer_beam_t* a, int it, asr_stream_t stream) {
  const int rc = beam_args_check(a);
  return rc ? rc : launch_step<false>(a, it, NoWlm(), stream);
}

extern "C" int asr_transducer_beam_cell_f32(const asr_transducer_beam_t* a, const float* gates, float* h, float* c, asr_stream_t stream) {
  const int rc = beam_args_check(a);
  if (rc) return rc;
  if (!gates || !h || !c) return ASR_E_ARG;
  const BeamWs w = beam_ws(a->ws, a->B, a->T, a->K, a->L, a->P);
  const int64_t total = (int64_t)a->B * a->K * a->P;
  hipLaunchKernelGGL(rnnt_beam_cell_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, total, a->E,
                     a->P, gates, (const float*)a->xh, (const float*)w.cg, (const int32_t*)w.advance, h, c);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_transducer_beam_backtrace_f32(const asr_transducer_beam_t* a, int32_t* hyp, int32_t* hyp_len, float* score,
                                           float* rnnt_score, float* lm_score, asr_stream_t stream) {
  const int rc = beam_args_check(a);
  return rc ? rc : launch_backtrace<false>(a, hyp, hyp_len, score, rnnt_score, lm_score, NoWlm(), nullptr, stream);
}

extern "C" int asr_transducer_wbeam_ws_bytes(int B, int K, int64_t* ws_bytes) {
  if (!ws_bytes || B <= 0) return ASR_E_ARG;
  if (K < 1 || K > kKmax) return ASR_E_SHAPE;
  *ws_bytes = wbeam_ws_bytes(B, K);
  return 0;
}

extern "C" int asr_transducer_wbeam_init_f32(const asr_transducer_beam_t* a, const asr_word_lm_t* lm, float alpha, float beta,
                                             int eos_term, int lexicon_only, void* wws, int64_t wws_bytes, int bos,
                                             asr_stream_t stream) {
  BeamWlm g;
  const int rc = wbeam_args(a, lm, alpha, beta, eos_term, lexicon_only, wws, wws_bytes, &g);
  return rc ? rc : launch_init<true>(a, bos, g, stream);
}

extern "C" int asr_transducer_wbeam_step_f32(const asr_transducer_beam_t* a, const asr_word_lm_t* lm, float alpha, float beta,
                                             int eos_term, int lexicon_only, void* wws, int64_t wws_bytes, int it,
                                             asr_stream_t stream) {
  BeamWlm g;
  const int rc = wbeam_args(a, lm, alpha, beta, eos_term, lexicon_only, wws, wws_bytes, &g);
  return rc ? rc : launch_step<true>(a, it, g, stream);
}

extern "C" int asr_transducer_wbeam_backtrace_f32(const asr_transducer_beam_t* a, const asr_word_lm_t* lm, float alpha, float beta,
                                                  int eos_term, int lexicon_only, void* wws, int64_t wws_bytes, int32_t* hyp,
                                                  int32_t* hyp_len, float* score, float* rnnt_score, float* lm_score,
                                                  int32_t* n_words, asr_stream_t stream) {
  BeamWlm g;
  const int rc = wbeam_args(a, lm, alpha, beta, eos_term, lexicon_only, wws, wws_bytes, &g);
  return rc ? rc : launch_backtrace<true>(a, hyp, hyp_len, score, rnnt_score, lm_score, g, n_words, stream);
}
