// gtc_nbest.hip — the n-best list of the CTC prefix beam search compiled into graph CTC tables on the device:
// per row the weighted prefix tree gtc.Graph.from_nbest builds on the host, written into one asr_gtc_graphs_t table as
// gtc._concat lays it out, element for element.  Integer work and float64 weights only: nothing to reorder, the same bits
// in every run, a row's graph a function of that row alone.
//   gtc_nbest_count_kernel   one workgroup per row: the row's plan, then its node and arc counts
//   gtc_nbest_fill_kernel    one workgroup per row: the plan again, the sum of the rows in front (the exclusive scan, each
//                            workgroup for itself), then every array of the row
// The plan of a row (K <= 16 hypotheses):
//   1. live slots (hyp_len >= 0 and score > -inf), their 16 x 16 table of longest common prefixes
//   2. admission in slot order while the tree stays within 1023 trie nodes: hypothesis k adds len_k - max over the admitted
//      j < k of lcp(j, k) nodes; the first that does not fit and every slot behind it are dropped
//   3. the weights: log-softmax of temperature * score over the admitted slots, float64
//   4. the admitted hypotheses sorted lexicographically (a prefix before its extensions, duplicates in slot order).  With
//      prev_i = lcp(sorted i-1, sorted i) a trie node exists at (i, depth d) iff prev_i <= d < len_i, and the nodes of one
//      depth, in the order of i, are in breadth-first order with children in token order.  So the number of node (i, d) is
//      1 + sum_i' max(0, min(len_i', d) - prev_i') + #{i' < i : prev_i' <= d < len_i'}: counts over at most 16 hypotheses.
//   5. per trie node its token, parent, first child, child count, the children with another token (the skip arcs) and
//      the joined weight of the hypotheses that end there (logaddexp in float64, ascending slot order)
//   6. an exclusive scan of the arc counts over the trie nodes
// Trie node u gives the token node 2u - 1 and the blank node 2u, node 0 is the root's blank; every arc weighs 0.
// Trust: the tokens of live hypotheses lie in 1 .. V-1 (they come from asr_ctc_beam_f32); a token outside is written into
// lab as it stands and is the loss kernels' to meet.  No index here is formed from a token: whatever the tokens are, every
// read and write of these kernels stays inside the caller's arrays.
#include "seq_common.h"

// The weights are gtc.nbest_weights' operations one by one: a product rounded, then a difference rounded.  Contracted into
// one fused multiply-add, temperature * score - lse of a row's only hypothesis is the product's rounding error, not 0.
#pragma clang fp contract(off)

namespace {

constexpr int kNbK = ASR_BEAM_KMAX;
constexpr int kNbMaxU = (ASR_GTC_MAX_NODES - 1) / 2;       // trie nodes beyond the root
constexpr int kNbSlots = kNbMaxU + 1;                      // with the root
constexpr int kNbThreads = 256;
constexpr int kNbPer = kNbSlots / kNbThreads;              // trie nodes per thread in the scan
constexpr int kNbTokShift = 11;                            // sort key = (token << 11) | trie node
constexpr int kNbHeadShift = 12;                           // head entry = (first << 12) | run (gtc.hip's kGtcHeadShift)
static_assert(kNbSlots == kNbPer * kNbThreads, "the scan gives every thread the same number of trie nodes");
static_assert(kNbMaxU < (1 << kNbTokShift), "a trie node must fit the low bits of a sort key");
static_assert(kNbK * kNbK <= kNbThreads, "one thread per pair of hypotheses");

struct NbPlan {
  int lcp[kNbK][kNbK];
  int len[kNbK];            // by slot: the length of an admitted hypothesis, -1 otherwise
  double w[kNbK];           // by slot: the log weight in the graph
  int sorted[kNbK];         // sorted position -> slot
  int slen[kNbK], sprev[kNbK];
  int M, U, A;
  int tok[kNbSlots], par[kNbSlots], fc[kNbSlots], nc[kNbSlots], nd[kNbSlots];
  float end[kNbSlots];
  int outo[kNbSlots], ino[kNbSlots];          // the arcs in front of the pair (2u - 1, 2u), inside the graph
  unsigned key[kNbSlots];
  int scan[kNbThreads];
  int base[2];
};

__device__ __forceinline__ double nb_logaddexp(double a, double b) {
  if (a == -INFINITY) return b;
  if (b == -INFINITY) return a;
  const double m = a > b ? a : b, n = a > b ? b : a;
  return m + log1p(exp(n - m));
}

// the breadth-first number of the trie node at (sorted hypothesis i, depth d)
__device__ __forceinline__ int nb_number(const NbPlan& P, int i, int d) {
  int u = 1;
  for (int j = 0; j < P.M; ++j) {
    const int lo = P.sprev[j], hi = P.slen[j] < d ? P.slen[j] : d;
    if (hi > lo) u += hi - lo;
    if (j < i && lo <= d && d < P.slen[j]) ++u;
  }
  return u;
}

// The plan of row b in P.  log_weights / dropped: written when not NULL.  Every thread of the workgroup calls it.
__device__ void nb_plan(NbPlan& P, int K, int L, const int32_t* __restrict__ hyp, const int32_t* __restrict__ hyp_len,
                        const float* __restrict__ score, double temperature, double* __restrict__ log_weights,
                        int32_t* __restrict__ dropped) {
  const int tid = threadIdx.x;
  if (tid < K) {
    const int hl = hyp_len[tid];
    const bool live = hl >= 0 && score[tid] > -INFINITY;
    P.len[tid] = live ? (hl < L ? hl : L) : -1;
  }
  __syncthreads();
  if (tid < K * K) {
    const int j = tid / K, k = tid % K;
    if (j < k) {
      int l = 0;
      if (P.len[j] >= 0 && P.len[k] >= 0) {
        const int n = P.len[j] < P.len[k] ? P.len[j] : P.len[k];
        const int32_t* hj = hyp + (int64_t)j * L;
        const int32_t* hk = hyp + (int64_t)k * L;
        while (l < n && hj[l] == hk[l]) ++l;
      }
      P.lcp[j][k] = P.lcp[k][j] = l;
    }
  }
  __syncthreads();
  if (tid == 0) {
    int nodes = 0, lost = 0, M = 0;
    unsigned adm = 0;
    bool stop = false;
    for (int k = 0; k < K; ++k) {
      const int lk = P.len[k];
      if (lk < 0) continue;
      if (!stop) {
        int best = 0;
        for (int j = 0; j < k; ++j)
          if (((adm >> j) & 1u) && P.lcp[j][k] > best) best = P.lcp[j][k];
        if (nodes + (lk - best) > kNbMaxU) {
          stop = true;
        } else {
          adm |= 1u << k;
          nodes += lk - best;
          ++M;
        }
      }
      if (stop) {
        ++lost;
        P.len[k] = -1;
      }
    }
    double m = -INFINITY;
    for (int k = 0; k < K; ++k)
      if ((adm >> k) & 1u) {
        const double s = temperature * (double)score[k];
        m = s > m ? s : m;
      }
    double sum = 0.0;
    for (int k = 0; k < K; ++k)
      if ((adm >> k) & 1u) sum += exp(temperature * (double)score[k] - m);
    const double lse = M ? m + log(sum) : 0.0;
    for (int k = 0; k < K; ++k) {
      const double lw = ((adm >> k) & 1u) ? temperature * (double)score[k] - lse : -INFINITY;
      P.w[k] = lw;
      if (log_weights) log_weights[k] = lw;
    }
    if (dropped) *dropped = lost;
    if (M == 0) {                               // no hypothesis left: the empty hypothesis at weight 0, in slot 0
      P.len[0] = 0;
      P.w[0] = 0.0;
      M = 1;
    }
    P.M = M;
    P.U = nodes;
  }
  __syncthreads();
  if (tid < K && P.len[tid] >= 0) {
    int rank = 0;
    const int lk = P.len[tid];
    for (int j = 0; j < K; ++j) {
      const int lj = P.len[j];
      if (j == tid || lj < 0) continue;
      const int l = P.lcp[j][tid];
      bool less;                                // hypothesis j sorts in front of hypothesis tid
      if (l == lj && l == lk) less = j < tid;
      else if (l == lj) less = true;
      else if (l == lk) less = false;
      else less = hyp[(int64_t)j * L + l] < hyp[(int64_t)tid * L + l];
      rank += less ? 1 : 0;
    }
    P.sorted[rank] = tid;
  }
  __syncthreads();
  const int M = P.M, U = P.U;
  if (tid < M) {
    P.slen[tid] = P.len[P.sorted[tid]];
    P.sprev[tid] = tid ? P.lcp[P.sorted[tid - 1]][P.sorted[tid]] : 0;
  }
  __syncthreads();
  if (tid == 0) {                               // the root
    double e = -INFINITY;
    int nc = 0, fc = 0;
    for (int i = 0; i < M; ++i) {
      if (P.slen[i] == 0) {
        e = nb_logaddexp(e, P.w[P.sorted[i]]);
      } else if (P.sprev[i] == 0) {
        if (!nc) fc = nb_number(P, i, 0);
        ++nc;
      }
    }
    P.tok[0] = 0, P.par[0] = 0, P.fc[0] = fc, P.nc[0] = nc, P.nd[0] = 0, P.end[0] = (float)e;
  }
  for (int i = 0; i < M; ++i) {
    const int32_t* hi = hyp + (int64_t)P.sorted[i] * L;
    for (int d = P.sprev[i] + tid; d < P.slen[i]; d += kNbThreads) {
      const int u = nb_number(P, i, d);
      if (u < 1 || u > U) continue;             // (cannot be: the numbers of a tree of U nodes are 1 .. U)
      const int tok = hi[d];
      int j = i;
      while (j > 0 && P.sprev[j] >= d) --j;
      double e = P.slen[i] == d + 1 ? P.w[P.sorted[i]] : -INFINITY;
      int nc = 0, fc = 0, nd = 0;
      if (P.slen[i] > d + 1) {
        nc = 1, fc = nb_number(P, i, d + 1);
        nd += hi[d + 1] != tok ? 1 : 0;
      }
      for (int i2 = i + 1; i2 < M && P.sprev[i2] >= d + 1; ++i2) {
        if (P.slen[i2] == d + 1) {
          e = nb_logaddexp(e, P.w[P.sorted[i2]]);
        } else if (P.sprev[i2] == d + 1) {
          if (!nc) fc = nb_number(P, i2, d + 1);
          ++nc;
          nd += hyp[(int64_t)P.sorted[i2] * L + d + 1] != tok ? 1 : 0;
        }
      }
      P.tok[u] = tok, P.par[u] = d ? nb_number(P, j, d - 1) : 0, P.fc[u] = fc, P.nc[u] = nc, P.nd[u] = nd, P.end[u] = (float)e;
    }
  }
  __syncthreads();
  // the arcs in front of every trie node: out arcs in the high half of a word, in arcs in the low half (both below 2^13)
  int mine[kNbPer], sum = 0;
#pragma unroll
  for (int q = 0; q < kNbPer; ++q) {
    const int u = tid * kNbPer + q;
    int v = 0;
    if (u == 0) {
      v = ((1 + P.nc[0]) << 16) | 1;
    } else if (u <= U) {
      const int p = P.par[u];
      v = ((3 + P.nc[u] + P.nd[u]) << 16) | (4 + ((p != 0 && P.tok[p] != P.tok[u]) ? 1 : 0));
    }
    mine[q] = v;
    sum += v;
  }
  P.scan[tid] = sum;
  __syncthreads();
  for (int off = 1; off < kNbThreads; off <<= 1) {
    const int v = tid >= off ? P.scan[tid - off] : 0;
    __syncthreads();
    P.scan[tid] += v;
    __syncthreads();
  }
  int at = tid ? P.scan[tid - 1] : 0;
#pragma unroll
  for (int q = 0; q < kNbPer; ++q) {
    const int u = tid * kNbPer + q;
    P.outo[u] = at >> 16;
    P.ino[u] = at & 0xffff;
    at += mine[q];
  }
  if (tid == kNbThreads - 1) P.A = at & 0xffff;
  __syncthreads();
}

__global__ __launch_bounds__(kNbThreads) void gtc_nbest_count_kernel(int K, int L, const int32_t* __restrict__ hyp,
                                                                     const int32_t* __restrict__ hyp_len,
                                                                     const float* __restrict__ score, double temperature,
                                                                     int32_t* __restrict__ cnt) {
  __shared__ NbPlan P;
  const int b = blockIdx.x;
  nb_plan(P, K, L, hyp + (int64_t)b * K * L, hyp_len + (int64_t)b * K, score + (int64_t)b * K, temperature, nullptr, nullptr);
  if (threadIdx.x == 0) {
    cnt[2 * b] = 2 * P.U + 1;
    cnt[2 * b + 1] = P.A;
  }
}

__global__ __launch_bounds__(kNbThreads) void gtc_nbest_fill_kernel(
    int B, int K, int L, int V, const int32_t* __restrict__ hyp, const int32_t* __restrict__ hyp_len,
    const float* __restrict__ score, double temperature, const int32_t* __restrict__ cnt, int32_t* __restrict__ node_off,
    int32_t* __restrict__ lab, float* __restrict__ start, float* __restrict__ fin, int32_t* __restrict__ in_ptr,
    int32_t* __restrict__ in_src, float* __restrict__ in_w, int32_t* __restrict__ out_ptr, int32_t* __restrict__ out_dst,
    float* __restrict__ out_w, int32_t* __restrict__ order, int32_t* __restrict__ head, int32_t* __restrict__ graph_of,
    double* __restrict__ log_weights, int32_t* __restrict__ dropped) {
  __shared__ NbPlan P;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < 2) P.base[tid] = 0;
  nb_plan(P, K, L, hyp + (int64_t)b * K * L, hyp_len + (int64_t)b * K, score + (int64_t)b * K, temperature,
          log_weights + (int64_t)b * K, dropped + b);
  // the rows in front: integer sums, any order
  int sn = 0, sa = 0;
  for (int r = tid; r < b; r += kNbThreads) {
    sn += cnt[2 * r];
    sa += cnt[2 * r + 1];
  }
  if (sn | sa) {
    atomicAdd(&P.base[0], sn);
    atomicAdd(&P.base[1], sa);
  }
  __syncthreads();
  const int n0 = P.base[0], a0 = P.base[1], U = P.U, N = 2 * U + 1, A = P.A;
  if (tid == 0) {
    node_off[b] = n0;
    if (b == B - 1) node_off[B] = n0 + N;
    graph_of[b] = b;
    in_ptr[n0 + N] = a0 + A;
    out_ptr[n0 + N] = a0 + A;
    // the root's blank
    lab[n0] = 0, start[n0] = 0.f, fin[n0] = P.end[0];
    in_ptr[n0] = a0, in_src[a0] = 0, in_w[a0] = 0.f;
    out_ptr[n0] = a0, out_dst[a0] = 0, out_w[a0] = 0.f;
    for (int c = 0; c < P.nc[0]; ++c) out_dst[a0 + 1 + c] = 2 * (P.fc[0] + c) - 1, out_w[a0 + 1 + c] = 0.f;
    order[n0] = 0;
    head[(int64_t)b * V] = U + 1;               // the blanks lead the sorted list: first 0, run U + 1
  }
  for (int u = 1 + tid; u <= U; u += kNbThreads) {
    const int gl = n0 + 2 * u - 1, gb = gl + 1, p = P.par[u], tok = P.tok[u];
    const bool diff = p != 0 && P.tok[p] != tok;
    lab[gl] = tok, lab[gb] = 0;
    start[gl] = p == 0 ? 0.f : -INFINITY, start[gb] = -INFINITY;
    fin[gl] = fin[gb] = P.end[u];
    int k = a0 + P.ino[u];
    in_ptr[gl] = k;
    if (diff) in_src[k] = 2 * p - 1, in_w[k++] = 0.f;
    in_src[k] = 2 * p, in_w[k++] = 0.f;
    in_src[k] = 2 * u - 1, in_w[k++] = 0.f;
    in_ptr[gb] = k;
    in_src[k] = 2 * u - 1, in_w[k++] = 0.f;
    in_src[k] = 2 * u, in_w[k++] = 0.f;
    k = a0 + P.outo[u];
    out_ptr[gl] = k;
    out_dst[k] = 2 * u - 1, out_w[k++] = 0.f;
    out_dst[k] = 2 * u, out_w[k++] = 0.f;
    const int fc = P.fc[u], nc = P.nc[u];
    for (int c = fc; c < fc + nc; ++c)
      if (P.tok[c] != tok) out_dst[k] = 2 * c - 1, out_w[k++] = 0.f;
    out_ptr[gb] = k;
    out_dst[k] = 2 * u, out_w[k++] = 0.f;
    for (int c = fc; c < fc + nc; ++c) out_dst[k] = 2 * c - 1, out_w[k++] = 0.f;
    order[n0 + u] = 2 * u;                      // the blanks, ascending
  }
  // the token nodes sorted by (token, node): a bitonic sort of distinct keys
  int P2 = 1;
  while (P2 < U) P2 <<= 1;
  for (int r = tid; r < P2; r += kNbThreads) P.key[r] = r < U ? (((unsigned)P.tok[r + 1] << kNbTokShift) | (unsigned)(r + 1)) : 0xffffffffu;
  __syncthreads();
  for (int kk = 2; kk <= P2; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int r = tid; r < P2; r += kNbThreads) {
        const int x = r ^ j;
        if (x > r) {
          const unsigned a = P.key[r], c = P.key[x];
          if ((a > c) == ((r & kk) == 0)) P.key[r] = c, P.key[x] = a;
        }
      }
      __syncthreads();
    }
  }
  for (int r = tid; r < U; r += kNbThreads) order[n0 + U + 1 + r] = 2 * (int)(P.key[r] & ((1u << kNbTokShift) - 1)) - 1;
  for (int v = 1 + tid; v < V; v += kNbThreads) {
    int at[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {               // the first key at or above (v + s) << 11
      const unsigned want = (unsigned)(v + s) << kNbTokShift;
      int lo = 0, hi = U;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (P.key[mid] < want) lo = mid + 1;
        else hi = mid;
      }
      at[s] = lo;
    }
    head[(int64_t)b * V + v] = at[1] > at[0] ? (((U + 1 + at[0]) << kNbHeadShift) | (at[1] - at[0])) : 0;
  }
}

int nb_caps(int B, int K, int L, int V, int64_t* cap_nodes, int64_t* cap_arcs) {
  if (B <= 0 || K <= 0 || L <= 0 || V <= 0) return ASR_E_ARG;
  if (K > kNbK || V < 2 || V > (1 << 20)) return ASR_E_SHAPE;
  const int64_t full = 2 * (int64_t)K * L + 1;
  *cap_nodes = full < ASR_GTC_MAX_NODES ? full : ASR_GTC_MAX_NODES;
  *cap_arcs = 3 * *cap_nodes;
  if ((int64_t)B * *cap_arcs > INT_MAX / 2 || (int64_t)B * V > INT_MAX / 2 || (int64_t)B * K * L > INT_MAX / 2) return ASR_E_SHAPE;
  return 0;
}

}  // namespace

extern "C" int asr_nbest_gtc_bytes(int B, int K, int L, int V, int32_t* cap_nodes, int32_t* cap_arcs, int64_t* ws_bytes) {
  if (!cap_nodes || !cap_arcs || !ws_bytes) return ASR_E_ARG;
  int64_t cn = 0, ca = 0;
  const int rc = nb_caps(B, K, L, V, &cn, &ca);
  if (rc) return rc;
  *cap_nodes = (int32_t)cn;
  *cap_arcs = (int32_t)ca;
  *ws_bytes = 8 * (int64_t)B;
  return 0;
}

extern "C" int asr_nbest_gtc_f32(int B, int K, int L, int V, const int32_t* hyp, const int32_t* hyp_len, const float* score,
                                 double temperature, const asr_gtc_graphs_t* table, int32_t* graph_of, double* log_weights,
                                 int32_t* dropped, void* ws, int64_t ws_bytes, asr_stream_t stream) {
  if (!hyp || !hyp_len || !score || !table || !graph_of || !log_weights || !dropped || !ws) return ASR_E_ARG;
  int64_t cn = 0, ca = 0;
  const int rc = nb_caps(B, K, L, V, &cn, &ca);
  if (rc) return rc;
  if (!(temperature >= 0.0) || !(temperature < (double)INFINITY)) return ASR_E_ARG;
  const asr_gtc_graphs_t& G = *table;
  if (G.V != V || G.G != B || G.max_nodes != cn || G.max_arcs != ca || ((uintptr_t)ws & 3) || ws_bytes < 8 * (int64_t)B)
    return ASR_E_ARG;
  if (!G.node_off || !G.lab || !G.start || !G.fin || !G.in_ptr || !G.in_src || !G.in_w || !G.out_ptr || !G.out_dst || !G.out_w ||
      !G.order || !G.head)
    return ASR_E_ARG;
  int32_t* cnt = (int32_t*)ws;
  hipLaunchKernelGGL(gtc_nbest_count_kernel, dim3(B), dim3(kNbThreads), 0, (hipStream_t)stream, K, L, hyp, hyp_len, score,
                     temperature, cnt);
  ASR_CHECK_LAUNCH();
  hipLaunchKernelGGL(gtc_nbest_fill_kernel, dim3(B), dim3(kNbThreads), 0, (hipStream_t)stream, B, K, L, V, hyp, hyp_len, score,
                     temperature, cnt, (int32_t*)G.node_off, (int32_t*)G.lab, (float*)G.start, (float*)G.fin,
                     (int32_t*)G.in_ptr, (int32_t*)G.in_src, (float*)G.in_w, (int32_t*)G.out_ptr, (int32_t*)G.out_dst,
                     (float*)G.out_w, (int32_t*)G.order, (int32_t*)G.head, graph_of, log_weights, dropped);
  ASR_CHECK_LAUNCH();
  return 0;
}
