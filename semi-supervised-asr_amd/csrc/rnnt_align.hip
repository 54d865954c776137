// rnnt_align.hip — forced alignment on the transducer head's lattice: the Viterbi (max-product) companion of
// rnnt.hip's loss forward, on the same inputs.  The conventions are seq_common.h's and rnnt.hip's: blank = 0, x = z - lse,
// a node is (b, t, u) with t < T_b, u <= U_b, node matrices [B][T][U + 1] row-major, every offset 64-bit, padding nodes
// never read.  No floating-point atomics, adds and compares only behind the row pass: the same bits in every run.
//   rnnt_align_node_kernel   one wave per node: the row's max / sum-exp (seq_common.h), then lane 0 writes the node's two
//                            emissions lp_0(t, u) and lp_{y_{u+1}}(t, u) - no [.., V] log-prob tensor exists
//   rnnt_align_chain_kernel  one workgroup per utterance, rnnt_alpha_kernel's geometry (one wave up to 64 label positions,
//                            256 threads beyond, positions strided over the workgroup above 256).  Three phases:
//                              chain      v by anti-diagonals t + u = d with max in place of logaddexp; two diagonals in
//                                         LDS, one barrier per diagonal, the next diagonal's two emissions loaded before
//                                         it.  Each node's choice is one bit (1: it was entered by its label arc from
//                                         (t, u-1); 0: by the blank arc from (t-1, u), which also wins a tie); a wave ballot
//                                         gives the 64-bit word of (diagonal, u / 64), written by one lane to the workspace
//                              backtrace  wave 0 walks from (T_b-1, U_b) to (0, 0): the words of 64 diagonals are loaded at
//                                         once (a lane per diagonal) and handed round by shuffle, so the walk waits for
//                                         memory once per 64 steps; lane 0 writes emit_frame and frame_labels
//                              output     parallel over labels and frames: token_logp, blank_logp, and the padding
#include "seq_common.h"

namespace {

constexpr int kMaxU = ASR_RNNT_MAX_LABELS;

typedef unsigned long long u64;

struct RnntAlignWs {
  u64* bp;         // [B][T + U][W]       back-pointer words by (diagonal, u / 64), W = ceil((U + 1) / 64)
  float* lpb;      // [B][T][U + 1]       lp_0(t, u)
  float* lpy;      // [B][T][U + 1]       lp_{y_{u+1}}(t, u), u < U_b
  int64_t bytes;
};

RnntAlignWs rnnt_align_ws(void* base, int B, int T, int U1) {
  const int64_t W = (U1 + 63) / 64;
  const int64_t n_bp = (int64_t)B * (T + U1 - 1) * W, n_node = round64((int64_t)B * T * U1);
  RnntAlignWs w;
  w.bp = (u64*)base;                                         // (first: 8-byte aligned wherever the workspace is)
  w.lpb = (float*)(w.bp + n_bp);
  w.lpy = w.lpb + n_node;
  w.bytes = 8 * n_bp + 4 * 2 * n_node;
  return w;
}

// asr_rnnt_ws_bytes's bounds on the node matrix (its J taken as 4): a wave per node in workgroups of four
int rnnt_align_shape_check(int B, int T, int U, int V) {
  if (B <= 0 || T <= 0 || U < 0 || V <= 0) return ASR_E_ARG;
  if (V < 2 || U > kMaxU) return ASR_E_SHAPE;
  const __int128 nodes = (__int128)B * T * (U + 1);
  if ((nodes + 3) / 4 > 0x7fffffffLL || nodes * (V > 4 ? V : 4) > ((__int128)1 << 40)) return ASR_E_SHAPE;
  return 0;
}

__global__ __launch_bounds__(256) void rnnt_align_node_kernel(int64_t nodes, int T, int U1, int V, const float* __restrict__ z,
                                                              int64_t ld, const int32_t* __restrict__ lens,
                                                              const int64_t* __restrict__ labels,
                                                              const int32_t* __restrict__ offs, float* __restrict__ lpb,
                                                              float* __restrict__ lpy) {
  const int lane = threadIdx.x & 63;
  const int64_t node = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (node >= nodes) return;
  const int u = (int)(node % U1);
  const int64_t bt = node / U1;
  const int t = (int)(bt % T), b = (int)(bt / T);
  const int o0 = offs[b], n = offs[b + 1] - o0;
  const int L = n < 0 ? 0 : (n > U1 - 1 ? U1 - 1 : n);
  if (t >= clamp_len(lens[b], T) || u > L) return;           // padding is never read
  const float* zr = z + node * ld;
  float mx, se;
  wave_row_max_sumexp(zr, V, lane, mx, se);
  if (lane == 0) {
    const float ls = mx + logf(se);
    lpb[node] = zr[0] - ls;
    if (u < L) {
      const int64_t v = labels[o0 + u];
      lpy[node] = zr[(v < 1 || v >= V) ? 1 : (int)v] - ls;   // (an utterance with such a label is not aligned: not read)
    }
  }
}

// the two emissions the nodes of diagonal d at this thread's positions are entered with (absent: not read)
template <int NS>
__device__ __forceinline__ void fetch_diagonal(int d, int len, int L, int U1, const float* __restrict__ lpb,
                                               const float* __restrict__ lpy, float (&eb)[NS], float (&ey)[NS]) {
  const int ulo = d - (len - 1) > 0 ? d - (len - 1) : 0, uhi = d < L ? d : L;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int u = threadIdx.x + i * blockDim.x, t = d - u;
    eb[i] = 0.f;
    ey[i] = 0.f;
    if (u >= ulo && u <= uhi) {
      if (t > 0) eb[i] = lpb[(int64_t)(t - 1) * U1 + u];
      if (u > 0) ey[i] = lpy[(int64_t)t * U1 + (u - 1)];
    }
  }
}

// v(0, 0) = 0; v(t, u) = max(v(t-1, u) + lp_0(t-1, u), v(t, u-1) + lp_{y_u}(t, u-1)); the blank arc wins a tie
template <int NS>
__global__ __launch_bounds__(256) void rnnt_align_chain_kernel(int T, int U1, int V, const int32_t* __restrict__ lens,
                                                               const int64_t* __restrict__ labels,
                                                               const int32_t* __restrict__ offs, float* __restrict__ score,
                                                               int32_t* emit_frame, float* __restrict__ token_logp,
                                                               int32_t* frame_labels, float* __restrict__ blank_logp,
                                                               RnntAlignWs w) {
  __shared__ float buf[2][kMaxU + 2];          // v of the previous / this diagonal at [u + 1]
  __shared__ int bad;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nwv = nt >> 6;
  const int o0 = offs[b], L = offs[b + 1] - o0;
  const int len = clamp_len(lens[b], T);
  int32_t* fl = frame_labels + (int64_t)b * T;
  float* bl = blank_logp + (int64_t)b * T;
  // a label outside [1, V), more labels than the launch holds, no frame: no alignment
  if (tid == 0) bad = (L < 0 || L > U1 - 1) ? 1 : 0;
  __syncthreads();
  if (!bad) {
    for (int i = tid; i < L; i += nt) {
      const int64_t v = labels[o0 + i];
      if (v < 1 || v >= V) atomicOr(&bad, 1);
    }
  }
  __syncthreads();
  if (bad || len == 0) {
    for (int t = tid; t < T; t += nt) {
      fl[t] = -1;
      bl[t] = 0.f;
    }
    for (int i = tid; i < L && emit_frame; i += nt) {        // (a call with U = 0 may come without the packed outputs)
      emit_frame[o0 + i] = -1;
      token_logp[o0 + i] = -INFINITY;
    }
    if (tid == 0) score[b] = -INFINITY;
    return;
  }
  const int W = (U1 + 63) >> 6;
  const float* lpb = w.lpb + (int64_t)b * T * U1;
  const float* lpy = w.lpy + (int64_t)b * T * U1;
  u64* bp = w.bp + (int64_t)b * (T + U1 - 1) * W;
  const int nd = len + L;                                    // diagonals 0 .. nd - 1
  float eb[NS], ey[NS], nb[NS], ny[NS];
  fetch_diagonal<NS>(1, len, L, U1, lpb, lpy, eb, ey);       // (nd == 1: every position is off diagonal 1, nothing is read)
  if (tid == 0) buf[0][1] = 0.f;
  __syncthreads();
  int p = 0;
  for (int d = 1; d < nd; ++d) {
    fetch_diagonal<NS>(d + 1, len, L, U1, lpb, lpy, nb, ny); // (d + 1 == nd: nothing is read)
    const int ulo = d - (len - 1) > 0 ? d - (len - 1) : 0, uhi = d < L ? d : L;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int u = tid + i * nt;
      bool take = false;
      if (u >= ulo && u <= uhi) {
        float v;
        if (u == d) {                                        // t = 0: the label arc alone
          v = buf[p][u] + ey[i];
          take = true;
        } else if (u == 0) {                                 // the blank arc alone
          v = buf[p][1] + eb[i];
        } else {
          const float cb = buf[p][u + 1] + eb[i], cy = buf[p][u] + ey[i];
          take = cy > cb;
          v = take ? cy : cb;
        }
        buf[p ^ 1][u + 1] = v;
      }
      const u64 m = __ballot(take);
      const int word = wave + i * nwv;                       // the wave's 64 positions of this round
      if (lane == 0 && word >= (ulo >> 6) && word <= (uhi >> 6)) bp[(int64_t)d * W + word] = m;
    }
    __syncthreads();
    p ^= 1;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      eb[i] = nb[i];
      ey[i] = ny[i];
    }
  }
  for (int t = len + tid; t < T; t += nt) {
    fl[t] = -1;
    bl[t] = 0.f;
  }
  // the backtrace: every lane of wave 0 walks, lane 0 writes.  A chunk is up to 64 steps from diagonal d down: lane i holds
  // the words of diagonal d - i at u / 64 and at u / 64 - 1 (64 steps lower u by less than 64).  A step moves along the
  // label arc only while u > 0 and along the blank arc only while t > 0, whatever a word holds: the walk stays on the lattice.
  if (wave == 0) {
    int t = len - 1, u = L;
    if (lane == 0) {
      score[b] = buf[p][L + 1] + lpb[(int64_t)(len - 1) * U1 + L];
      fl[len - 1] = L;
    }
    for (int d = t + u; d >= 1;) {
      const int w0 = u >> 6, dd = d - lane;
      u64 wa = 0, wc = 0;
      if (dd >= 1) {                                         // only words the chain has written
        const int lo = (dd - (len - 1) > 0 ? dd - (len - 1) : 0) >> 6, hi = (dd < L ? dd : L) >> 6;
        if (w0 >= lo && w0 <= hi) wa = bp[(int64_t)dd * W + w0];
        if (w0 - 1 >= lo && w0 - 1 <= hi) wc = bp[(int64_t)dd * W + (w0 - 1)];
      }
      const int n = d < 64 ? d : 64;
      for (int i = 0; i < n; ++i) {
        const u64 a = __shfl(wa, i, 64), c = __shfl(wc, i, 64);
        const u64 word = (u >> 6) == w0 ? a : c;
        if (u > 0 && (t == 0 || ((word >> (u & 63)) & 1))) {
          if (lane == 0) emit_frame[o0 + u - 1] = t;
          --u;
        } else {
          --t;
          if (lane == 0) fl[t] = u;
        }
      }
      d -= n;
    }
  }
  __syncthreads();
  for (int i = tid; i < L; i += nt) token_logp[o0 + i] = lpy[(int64_t)emit_frame[o0 + i] * U1 + i];
  for (int t = tid; t < len; t += nt) bl[t] = lpb[(int64_t)t * U1 + fl[t]];
}

}  // namespace

extern "C" int asr_transducer_align_ws_bytes(int B, int T, int U, int V, int64_t* ws_bytes) {
  if (!ws_bytes) return ASR_E_ARG;
  const int rc = rnnt_align_shape_check(B, T, U, V);
  if (rc) return rc;
  *ws_bytes = rnnt_align_ws(nullptr, B, T, U + 1).bytes;
  return 0;
}

extern "C" int asr_transducer_align_f32(int B, int T, int U, int V, const float* logits, int64_t ld, const int32_t* frame_lens,
                                  const int64_t* labels, const int32_t* label_offsets, float* score, int32_t* emit_frame,
                                  float* token_logp, int32_t* frame_labels, float* blank_logp, void* ws, int64_t ws_bytes,
                                  asr_stream_t stream) {
  if (!logits || !frame_lens || !label_offsets || !score || !frame_labels || !blank_logp || !ws) return ASR_E_ARG;
  if (U > 0 && (!labels || !emit_frame || !token_logp)) return ASR_E_ARG;
  const int rc = rnnt_align_shape_check(B, T, U, V);
  if (rc == ASR_E_ARG || ld < V) return ASR_E_ARG;
  if (rc) return rc;
  if ((((uintptr_t)ws) & 7u) != 0) return ASR_E_ALIGN;
  const RnntAlignWs w = rnnt_align_ws(ws, B, T, U + 1);
  if (ws_bytes < w.bytes) return ASR_E_ARG;
  const int64_t nodes = (int64_t)B * T * (U + 1);
  hipLaunchKernelGGL(rnnt_align_node_kernel, dim3((unsigned)((nodes + 3) / 4)), dim3(256), 0, (hipStream_t)stream, nodes, T,
                     U + 1, V, logits, ld, frame_lens, labels, label_offsets, w.lpb, w.lpy);
  ASR_CHECK_LAUNCH();
  if (U + 1 <= 256)
    hipLaunchKernelGGL(rnnt_align_chain_kernel<1>, dim3(B), dim3(U + 1 <= 64 ? 64 : 256), 0, (hipStream_t)stream, T, U + 1, V,
                       frame_lens, labels, label_offsets, score, emit_frame, token_logp, frame_labels, blank_logp, w);
  else
    hipLaunchKernelGGL(rnnt_align_chain_kernel<4>, dim3(B), dim3(256), 0, (hipStream_t)stream, T, U + 1, V, frame_lens, labels,
                       label_offsets, score, emit_frame, token_logp, frame_labels, blank_logp, w);
  ASR_CHECK_LAUNCH();
  return 0;
}
