// gtc.hip — graph CTC (GTC; Moritz et al. 2021): the CTC loss over a label graph, forward and backward.
// The supervision of an utterance is a graph of N nodes; node n carries a token lab[n] (0 = blank), a start weight and a
// final weight (fp32, finite or -inf), and arcs (m -> n, w) with a finite weight.  Self-loops are ordinary arcs.  With the
// conventions of seq_common.h (x = z - lse, ordered sums, log space) a path n_0 .. n_{T-1} along arcs scores
//   start[n_0] + sum_t x[t][lab[n_t]] + sum_{t >= 1} w(n_{t-1}, n_t) + fin[n_{T-1}]
// and nll = -logsumexp over all paths: a path sum, not a normalised probability.  The graphs come compiled from the host
// (gtc.py), several of them concatenated in one table, graph_of[b] names the graph of row b; rows may share a graph.
//   gtc_alpha_kernel  one workgroup per utterance (one wave when the largest graph has <= 64 nodes): alpha over the frames -
//                     a thread owns its nodes (strided when N exceeds the workgroup) and sums their INCOMING arcs with an
//                     online log-sum-exp in the table's arc order; the hand-off between frames goes through two rows of LDS
//                     with one barrier per frame, emissions are fetched two frames ahead
//   gtc_beta_kernel   the chain backwards over the OUTGOING arcs: the node occupancies, in linear space, from the shares
//                     the forward formed; writes the occupancy of (t, n) over what the forward stored there
//   gtc_grad_kernel   one wave per frame: the blank's run of the token-sorted node list is summed by the whole wave, every
//                     other token's run by the lane that owns the token, in ascending order
// Where the arcs live: the first kGtcRegArcs arcs of a node are read ONCE into registers in front of the chain, the rest
// are read from global memory (the L1 / L2 hold them) every frame.  A CTC lattice or an n-best prefix tree has at most
// three arcs into and four out of a node, so their chains touch no global arc at all.
#include "seq_common.h"

namespace {

constexpr int kGtcMaxN = ASR_GTC_MAX_NODES;
static_assert(kGtcMaxN <= kMaxS, "a graph must fit the LDS rows and launch_by_states of the CTC chains");
constexpr int kGtcRegArcs = 4;                 // arcs of a node that ride in registers
constexpr int kGtcHeadShift = 12;              // head entry = (first index in the sorted list << 12) | run length; 0: absent
static_assert(kGtcMaxN < (1 << kGtcHeadShift), "the run length must fit the low bits of a head entry");

struct GtcWs {
  float* lse;      // [B][T]
  float* raw;      // [B]            the nll before zero_infinity
  float* ab;       // [B][T][Np]     in_t(n), alpha_t(n) without its emission (frame 0: start[n]); after the backward's
                   //                first kernel the occupancy of (t, n);  Np = max_nodes
  int64_t bytes;
};

GtcWs gtc_ws(void* base, int B, int T, int Np) {
  const int64_t n_lse = round64((int64_t)B * T), n_raw = round64(B), n_ab = round64((int64_t)B * T * Np);
  GtcWs w;
  w.lse = (float*)base;
  w.raw = w.lse + n_lse;
  w.ab = w.raw + n_raw;
  w.bytes = 4 * (n_lse + n_raw + n_ab);
  return w;
}

// the online log-sum-exp of a node's arcs, one term at a time in the table's order: (m, s) = (largest term so far, sum of
// exp(term - m)).  A term of -inf (an unreachable predecessor, a padding arc) changes nothing, a single finite term comes
// back exactly (s = 1), and no -inf - -inf is ever formed.
__device__ __forceinline__ void lse_push(float& m, float& s, float v) {
  if (v > m) {
    s = s * expf(m - v) + 1.f;
    m = v;
  } else if (v > -INFINITY) {
    s += expf(v - m);
  }
}
__device__ __forceinline__ float lse_value(float m, float s) { return m > -INFINITY ? m + logf(s) : -INFINITY; }

template <int NS>
__global__ __launch_bounds__(256) void gtc_alpha_kernel(int T, const float* __restrict__ z, int64_t ld,
                                                        const int32_t* __restrict__ lens, asr_gtc_graphs_t G,
                                                        const int32_t* __restrict__ graph_of, int Np, int zero_inf,
                                                        float* __restrict__ nll, GtcWs w) {
  __shared__ float buf[2][kMaxS + 1];          // alpha of the previous / this frame
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int g = graph_of[b];
  const int n0 = G.node_off[g], N = G.node_off[g + 1] - n0;
  const int len = clamp_len(lens[b], T);
  if (len == 0 || N < 1 || N > Np || N > nt * NS) {          // no frame: no path (the sizes are the host's to keep)
    if (tid == 0) {
      w.raw[b] = INFINITY;
      nll[b] = zero_inf ? 0.f : INFINITY;
    }
    return;
  }
  const float* zb = z + (int64_t)b * T * ld;
  const float* lse = w.lse + (int64_t)b * T;
  float* ab = w.ab + (int64_t)b * T * Np;
  const int32_t* __restrict__ src = G.in_src;
  const float* __restrict__ aw = G.in_w;
  int li[NS], j0[NS], j1[NS], cs[NS][kGtcRegArcs];
  float cw[NS][kGtcRegArcs];
  bool act[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int n = tid + i * nt;
    act[i] = n < N;
    li[i] = act[i] ? G.lab[n0 + n] : 0;
    const int lo = act[i] ? G.in_ptr[n0 + n] : 0, hi = act[i] ? G.in_ptr[n0 + n + 1] : 0;
#pragma unroll
    for (int k = 0; k < kGtcRegArcs; ++k) {
      const bool have = lo + k < hi;
      cs[i][k] = have ? src[lo + k] : 0;
      cw[i][k] = have ? aw[lo + k] : -INFINITY;              // a padding arc: node 0 at weight -inf, a term of -inf
    }
    j0[i] = lo + kGtcRegArcs < hi ? lo + kGtcRegArcs : hi;
    j1[i] = hi;
  }
  // emissions of frames t, t + 1, t + 2 (raw logits; the frame's lse is subtracted where it is used)
  float z0[NS], z1[NS], z2[NS];
  float l0 = lse[0], l1 = len > 1 ? lse[1] : 0.f, l2 = 0.f;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    z0[i] = act[i] ? zb[li[i]] : 0.f;
    z1[i] = (act[i] && len > 1) ? zb[ld + li[i]] : 0.f;
    z2[i] = 0.f;
  }
  int p = 0;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int n = tid + i * nt;
    if (act[i]) {
      const float st = G.start[n0 + n];
      buf[0][n] = st + (z0[i] - l0);
      ab[n] = st;
    }
  }
  __syncthreads();
  for (int t = 1; t < len; ++t) {
    if (t + 1 < len) {
      l2 = lse[t + 1];
#pragma unroll
      for (int i = 0; i < NS; ++i)
        if (act[i]) z2[i] = zb[(int64_t)(t + 1) * ld + li[i]];
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int n = tid + i * nt;
      if (act[i]) {
        float m = -INFINITY, s = 0.f;
#pragma unroll
        for (int k = 0; k < kGtcRegArcs; ++k) lse_push(m, s, buf[p][cs[i][k]] + cw[i][k]);
        for (int j = j0[i]; j < j1[i]; ++j) lse_push(m, s, buf[p][src[j]] + aw[j]);
        const float in = lse_value(m, s);
        buf[p ^ 1][n] = in + (z1[i] - l1);
        ab[(int64_t)t * Np + n] = in;
      }
    }
    __syncthreads();
    p ^= 1;
    l1 = l2;
#pragma unroll
    for (int i = 0; i < NS; ++i) z1[i] = z2[i];
  }
  // nll = -logsum_n (alpha_{T-1}(n) + fin[n]): the first wave, lane-strided in ascending order, then the xor butterfly
  if (tid < 64) {
    float m = -INFINITY;
    for (int n = tid; n < N; n += 64) m = fmaxf(m, buf[p][n] + G.fin[n0 + n]);
    m = wave_max(m);
    float r = INFINITY;
    if (m > -INFINITY) {                                     // (wave-uniform)
      float se = 0.f;
      for (int n = tid; n < N; n += 64) se += expf((buf[p][n] + G.fin[n0 + n]) - m);
      r = -(m + logf(wave_sum(se)));
    }
    if (tid == 0) {
      w.raw[b] = r;
      nll[b] = (zero_inf && !(r < INFINITY)) ? 0.f : r;
    }
  }
}

// The backward chain.  What autograd does to the alpha recursion, in the open: the occupancy gamma_t(n) (the share of the path
// mass that sits in node n at frame t) goes backwards in LINEAR space,
//   gamma_{T-1}(n) = exp(alpha_{T-1}(n) + fin[n] + nll)
//   gamma_t(m)     = sum over the arcs (m -> n, w) of gamma_{t+1}(n) exp((alpha_t(m) + w) - in_{t+1}(n)),
// in_{t+1}(n) the log-sum-exp over n's incoming arcs that the forward stored, and alpha_t(m) + w the very term the forward
// pushed into it (alpha_t(m) = in_t(m) + x is formed again from the stored in_t(m) by the forward's own operations): each
// factor is a share the forward itself formed, at most 1, so the chain carries the forward's roundings instead of meeting
// them a second time.  A log-space beta and alpha + beta + nll (the star chains' exact-sum occupancy) is what
// was built first: it rounds alpha and beta at an ulp of their own magnitude, hundreds of nats wherever the best prefix so
// far is not the best path, and missed the gradient allowance 3 to 6 times over at |nll| > 2000.  An
// occupancy below the smallest float is 0: so is its share of the gradient.
template <int NS>
__global__ __launch_bounds__(256) void gtc_beta_kernel(int T, const float* __restrict__ z, int64_t ld,
                                                       const int32_t* __restrict__ lens, asr_gtc_graphs_t G,
                                                       const int32_t* __restrict__ graph_of, int Np, GtcWs w) {
  __shared__ float gam[2][kMaxS + 1];          // gamma of the next / this frame
  __shared__ float inl[2][kMaxS + 1];          // in of the next / this frame
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const float nllb = w.raw[b];
  if (!(nllb < INFINITY)) return;              // infeasible: the gradient kernel does not read the occupancies
  const int g = graph_of[b];
  const int n0 = G.node_off[g], N = G.node_off[g + 1] - n0;
  const int len = clamp_len(lens[b], T);
  if (len == 0 || N < 1 || N > Np || N > nt * NS) return;
  const float* zb = z + (int64_t)b * T * ld;
  const float* lse = w.lse + (int64_t)b * T;
  float* ab = w.ab + (int64_t)b * T * Np;
  const int32_t* __restrict__ dst = G.out_dst;
  const float* __restrict__ aw = G.out_w;
  int li[NS], j0[NS], j1[NS], cs[NS][kGtcRegArcs];
  float cw[NS][kGtcRegArcs];
  bool act[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int n = tid + i * nt;
    act[i] = n < N;
    li[i] = act[i] ? G.lab[n0 + n] : 0;
    const int lo = act[i] ? G.out_ptr[n0 + n] : 0, hi = act[i] ? G.out_ptr[n0 + n + 1] : 0;
#pragma unroll
    for (int k = 0; k < kGtcRegArcs; ++k) {
      const bool have = lo + k < hi;
      cs[i][k] = have ? dst[lo + k] : 0;
      cw[i][k] = have ? aw[lo + k] : -INFINITY;              // a padding arc: a share of exp(-inf) = 0
    }
    j0[i] = lo + kGtcRegArcs < hi ? lo + kGtcRegArcs : hi;
    j1[i] = hi;
  }
  // emissions and in of frames t, t - 1, t - 2
  float z0[NS], z1[NS], z2[NS], i0[NS], i1[NS], i2[NS];
  int t = len - 1;
  float l0 = lse[t], l1 = t > 0 ? lse[t - 1] : 0.f, l2 = 0.f;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int n = tid + i * nt;
    z0[i] = act[i] ? zb[(int64_t)t * ld + li[i]] : 0.f;
    i0[i] = act[i] ? ab[(int64_t)t * Np + n] : 0.f;
    z1[i] = (act[i] && t > 0) ? zb[(int64_t)(t - 1) * ld + li[i]] : 0.f;
    i1[i] = (act[i] && t > 0) ? ab[(int64_t)(t - 1) * Np + n] : 0.f;
    z2[i] = i2[i] = 0.f;
  }
  int p = 0;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int n = tid + i * nt;
    if (act[i]) {
      const float e = (i0[i] + (z0[i] - l0)) + G.fin[n0 + n];              // the forward's own alpha + fin
      const float ga = e > -INFINITY ? expf(e + nllb) : 0.f;
      gam[0][n] = ga;
      inl[0][n] = i0[i];
      ab[(int64_t)t * Np + n] = ga;
    }
  }
  __syncthreads();
  for (t = len - 2; t >= 0; --t) {
    if (t > 0) {
      l2 = lse[t - 1];
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const int n = tid + i * nt;
        if (act[i]) {
          z2[i] = zb[(int64_t)(t - 1) * ld + li[i]];
          i2[i] = ab[(int64_t)(t - 1) * Np + n];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int n = tid + i * nt;
      if (act[i]) {
        const float a = i1[i] + (z1[i] - l1);                              // alpha_t(n), the forward's bits
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < kGtcRegArcs; ++k) {
          const float gn = gam[p][cs[i][k]];
          if (gn > 0.f) s += gn * expf((a + cw[i][k]) - inl[p][cs[i][k]]);
        }
        for (int j = j0[i]; j < j1[i]; ++j) {
          const float gn = gam[p][dst[j]];
          if (gn > 0.f) s += gn * expf((a + aw[j]) - inl[p][dst[j]]);
        }
        gam[p ^ 1][n] = s;
        inl[p ^ 1][n] = i1[i];
        ab[(int64_t)t * Np + n] = s;
      }
    }
    __syncthreads();
    p ^= 1;
    l1 = l2;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      z1[i] = z2[i];
      i1[i] = i2[i];
    }
  }
}

// dz[b][t][k] = g_b (softmax_k - occ_k), occ_k = sum_{n : lab[n] = k} gamma_t(n) / all_t; gamma the occupancies of
// gtc_beta_kernel and all_t = sum_n gamma_t(n), which is 1 up to rounding: the occupancies of a frame are normalised by the
// frame's own total.  Zeros behind the utterance and for a row without a path, whatever zero_infinity.
__global__ __launch_bounds__(256) void gtc_grad_kernel(int B, int T, int V, const float* __restrict__ z, int64_t ld,
                                                       const int32_t* __restrict__ lens, asr_gtc_graphs_t G,
                                                       const int32_t* __restrict__ graph_of, int Np,
                                                       const float* __restrict__ gr, GtcWs w, float* __restrict__ dz,
                                                       int64_t lddz) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (int64_t)B * T) return;
  const int b = (int)(row / T), t = (int)(row % T);
  float* dzr = dz + row * lddz;
  const float nllb = w.raw[b];
  if (t >= lens[b] || !(nllb < INFINITY)) {
    for (int k = lane; k < V; k += 64) dzr[k] = 0.f;
    return;
  }
  const float* zr = z + row * ld;
  const float ls = w.lse[row], gb = gr[b];
  const int g = graph_of[b];
  const int n0 = G.node_off[g], N = G.node_off[g + 1] - n0;
  const float* abr = w.ab + row * Np;
  const int32_t* order = G.order + n0;
  const int32_t* head = G.head + (int64_t)g * V;
  // every node, then the blank's run: lane-strided in ascending order, then the xor butterfly
  float all = 0.f;
  for (int n = lane; n < N; n += 64) all += abr[n];
  all = wave_sum(all);
  const float inv = all > 0.f ? 1.f / all : 0.f;
  const int e0 = head[0], c0 = e0 & ((1 << kGtcHeadShift) - 1), h0 = e0 >> kGtcHeadShift;
  float blank = 0.f;
  for (int j = lane; j < c0; j += 64) blank += abr[order[h0 + j]];
  blank = wave_sum(blank);
  for (int k = lane; k < V; k += 64) {
    float sum = blank;
    if (k > 0) {
      const int e = head[k], c = e & ((1 << kGtcHeadShift) - 1), h = e >> kGtcHeadShift;
      sum = 0.f;
      for (int j = 0; j < c; ++j) sum += abr[order[h + j]];
    }
    dzr[k] = gb * (expf(zr[k] - ls) - sum * inv);
  }
}

int gtc_check(int B, int T, int V, int64_t ld, const asr_gtc_graphs_t* G, const void* ws, int64_t ws_bytes) {
  if (!G) return ASR_E_ARG;
  const int rc = ctc_shape_check(B, T, V, 0);
  if (rc == ASR_E_ARG || ld < V || !ws || G->G < 1 || G->max_nodes < 1 || G->max_arcs < 0 || G->V != V) return ASR_E_ARG;
  if (rc) return rc;
  if (G->max_nodes > kGtcMaxN || G->max_arcs > ASR_GTC_MAX_ARCS) return ASR_E_SHAPE;
  if (!G->node_off || !G->lab || !G->start || !G->fin || !G->in_ptr || !G->in_src || !G->in_w || !G->out_ptr || !G->out_dst ||
      !G->out_w || !G->order || !G->head)
    return ASR_E_ARG;
  if (((uintptr_t)ws & 3) || ws_bytes < gtc_ws(nullptr, B, T, G->max_nodes).bytes) return ASR_E_ARG;
  return 0;
}

}  // namespace

extern "C" int asr_gtc_ws_bytes(int B, int T, int V, int max_nodes, int64_t* ws_bytes) {
  if (B <= 0 || T <= 0 || V <= 0 || max_nodes < 1 || !ws_bytes) return ASR_E_ARG;
  if (V < 2 || max_nodes > kGtcMaxN) return ASR_E_SHAPE;
  *ws_bytes = gtc_ws(nullptr, B, T, max_nodes).bytes;
  return 0;
}

extern "C" int asr_gtc_loss_fwd(int B, int T, int V, const float* logits, int64_t ld, const int32_t* frame_lens,
                                const asr_gtc_graphs_t* graphs, const int32_t* graph_of, int zero_infinity, float* nll,
                                void* ws, int64_t ws_bytes, asr_stream_t stream) {
  if (!logits || !frame_lens || !graph_of || !nll) return ASR_E_ARG;
  const int rc = gtc_check(B, T, V, ld, graphs, ws, ws_bytes);
  if (rc) return rc;
  const int Np = graphs->max_nodes;
  const GtcWs w = gtc_ws(ws, B, T, Np);
  launch_frame_lse(B, T, V, logits, ld, frame_lens, w.lse, (hipStream_t)stream);
  ASR_CHECK_LAUNCH();
  launch_by_states(Np, gtc_alpha_kernel<1>, gtc_alpha_kernel<8>, B, (hipStream_t)stream, T, logits, ld, frame_lens, *graphs,
                   graph_of, Np, zero_infinity, nll, w);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_gtc_loss_bwd(int B, int T, int V, const float* logits, int64_t ld, const int32_t* frame_lens,
                                const asr_gtc_graphs_t* graphs, const int32_t* graph_of, int zero_infinity,
                                const float* grad_nll, void* ws, int64_t ws_bytes, float* dlogits, int64_t lddz,
                                asr_stream_t stream) {
  (void)zero_infinity;                          // a row without a path gets a zero gradient either way
  if (!logits || !frame_lens || !graph_of || !grad_nll || !dlogits || lddz < V) return ASR_E_ARG;
  const int rc = gtc_check(B, T, V, ld, graphs, ws, ws_bytes);
  if (rc) return rc;
  const int Np = graphs->max_nodes;
  const GtcWs w = gtc_ws(ws, B, T, Np);
  launch_by_states(Np, gtc_beta_kernel<1>, gtc_beta_kernel<8>, B, (hipStream_t)stream, T, logits, ld, frame_lens, *graphs,
                   graph_of, Np, w);
  ASR_CHECK_LAUNCH();
  const unsigned rows4 = (unsigned)(((int64_t)B * T + 3) / 4);
  hipLaunchKernelGGL(gtc_grad_kernel, dim3(rows4), dim3(256), 0, (hipStream_t)stream, B, T, V, logits, ld, frame_lens,
                     *graphs, graph_of, Np, grad_nll, w, dlogits, lddz);
  ASR_CHECK_LAUNCH();
  return 0;
}
