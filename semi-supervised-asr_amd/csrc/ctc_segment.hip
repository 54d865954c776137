// ctc_segment.hip — CTC segmentation (Kuerzinger et al. 2020): the Viterbi alignment of ctc_align.hip for a whole recording
// and its transcript of several utterances, up to ASR_CTC_SEG_MAX_LABELS labels, with free ends (audio before the first and
// after the last label costs nothing) and per-utterance begin / end / log-probability / confidence.  The conventions are
// seq_common.h's; its frame_lse_kernel runs first.  The recurrence, its arithmetic (one fp32 subtraction per emission, one
// fp32 add per cell) and its tie rule are ctc_align_kernel's, so with free_ends = 0 the shared outputs are that kernel's bits.
//   ctc_segment_kernel<K>  one workgroup per recording; thread i owns the K CONTIGUOUS states i K .. i K + K - 1 (K = 4: up to
//                          1 024 states on 64 .. 256 threads; K = 16: up to 16 384 states on 128 .. 1 024 threads).  Phases:
//     chain      the Viterbi row lives in registers (v[K], updated in place from the top state down).  K is even, so a
//                thread's first state is a blank (no skip) and its second state skips onto the state below the thread: the ONE
//                value a thread needs from its neighbour is that thread's top state of the frame before, exchanged through a
//                double-buffered LDS line - one barrier per frame.  The emissions of the two frames ahead are in flight
//                (K / 2 label logits and the blank per thread and frame).  A state's choice (0 stay, 1 from s-1, 2 from s-2)
//                is two bits; a thread's 2 K bits are formed in its own registers (the layout leaves no ballot to take) and
//                stored as one byte (K = 4) or one dword (K = 16): the frame's back-pointers are a bit row with state s at
//                bits 2 s, 2 s + 1, in the workspace, whatever K
//     backtrace  one wave, 32 frames per round: the state falls by at most 2 per frame, so the states of frames t .. t - 31
//                lie in 64-bit words W - 2 .. W of their rows (W = s >> 5 at frame t): lane 2 f + h loads words W - 2 h and
//                W - 2 h - 1 of frame t - f, all 128 loads in flight at once; the walk over the 32 frames is wave-uniform and
//                picks its word with v_readlane.  Lane i keeps the state of frame t - i: one coalesced store per round
//     output     parallel over the frames: path (-2 outside the text with free ends), x[t][path[t]] into the workspace, and
//                first / last of the label whose run starts / ends at the frame
//     sums       parallel over the labels: token_logp, by one lane in ascending frame order; then parallel over the
//                recording's utterances: begin, end, the sum and the windowed minimum mean of x[t][path[t]]
#include "seq_common.h"

namespace {

constexpr int kSegMaxL = ASR_CTC_SEG_MAX_LABELS;
constexpr int kSegThreads = 1024;
constexpr int kSegSmallStates = 1024;        // up to this many states: K = 4; beyond: K = 16
static_assert(16 * kSegThreads >= 2 * kSegMaxL + 1, "every state has a thread");
static_assert((kSegMaxL + 1) * 4 + 2 * (kSegThreads + 1) * 4 + 64 <= 64 * 1024, "the static LDS of a workgroup");

struct SegWs {
  u64* bp;         // [B][T][nw]   back-pointer bit rows: state s at bits 2 s, 2 s + 1; nw = ceil((2 max_label_len + 1) / 32)
  float* lse;      // [B][T]
  int* state;      // [B][T]       the state of every frame (the backtrace's output)
  float* fx;       // [B][T]       x[t][path[t]]
  int64_t nw;
  int64_t bytes;
};

SegWs seg_ws(void* base, int B, int T, int Lmax) {
  const int64_t n_bt = round64((int64_t)B * T);
  SegWs w;
  w.nw = (2 * (int64_t)Lmax + 1 + 31) / 32;
  w.bp = (u64*)base;                                        // (first: 8-byte aligned wherever the workspace is)
  w.lse = (float*)(w.bp + (int64_t)B * T * w.nw);
  w.state = (int*)(w.lse + n_bt);
  w.fx = (float*)(w.state + n_bt);
  w.bytes = 8 * (int64_t)B * T * w.nw + 4 * 3 * n_bt;
  return w;
}

template <int K> struct BpStore;
template <> struct BpStore<4> { typedef unsigned char type; };
template <> struct BpStore<16> { typedef unsigned int type; };

struct SegOut {
  int32_t* path;
  float* score;
  int32_t *first, *last;
  float* token_logp;
  int32_t *utt_begin, *utt_end;
  float *utt_logp, *utt_conf;
};

// a recording without an alignment: ctc_align_kernel's pattern, and its utterances
__device__ __forceinline__ void seg_infeasible(const SegOut& o, int b, int T, int o0, int L, int u0, int u1) {
  const int tid = threadIdx.x, nt = blockDim.x;
  int32_t* pathb = o.path + (int64_t)b * T;
  for (int t = tid; t < T; t += nt) pathb[t] = -1;
  for (int i = tid; i < L; i += nt) {
    o.first[o0 + i] = -1;
    o.last[o0 + i] = -1;
    o.token_logp[o0 + i] = -INFINITY;
  }
  for (int u = u0 + tid; u < u1; u += nt) {
    o.utt_begin[u] = -1;
    o.utt_end[u] = -1;
    o.utt_logp[u] = -INFINITY;
    o.utt_conf[u] = -INFINITY;
  }
}

template <int K>
__global__ __launch_bounds__(kSegThreads) void ctc_segment_kernel(int T, int V, const float* __restrict__ z, int64_t ld,
                                                                  const int32_t* __restrict__ lens,
                                                                  const int64_t* __restrict__ labels,
                                                                  const int32_t* __restrict__ offs, int Lmax, int free_ends,
                                                                  const int32_t* __restrict__ utt_offs,
                                                                  const int32_t* __restrict__ rec_utts, int window, SegOut o,
                                                                  SegWs w) {
  typedef typename BpStore<K>::type bp_t;
  constexpr int H = K / 2;
  __shared__ int lab[kSegMaxL + 1];
  __shared__ float edge[2][kSegThreads + 1];   // [.][i + 1]: thread i's top state, of the frame before / this frame; [.][0] -inf
  __shared__ float endv[2];
  __shared__ int bad, feasible;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & 63;
  const int o0 = offs[b], L = offs[b + 1] - o0, S = 2 * L + 1;
  const int u0 = rec_utts[b], u1 = rec_utts[b + 1];
  const int len = clamp_len(lens[b], T);
  int32_t* pathb = o.path + (int64_t)b * T;
  if (tid == 0) {
    edge[0][0] = -INFINITY;
    edge[1][0] = -INFINITY;
    endv[0] = -INFINITY;
    endv[1] = -INFINITY;
  }
  if (!ctc_load_labels(labels, o0, L, Lmax, V, lab, &bad) || len == 0) {
    seg_infeasible(o, b, T, o0, L, u0, u1);
    if (tid == 0) o.score[b] = -INFINITY;
    return;
  }
  const float* zb = z + (int64_t)b * T * ld;
  const float* lse = w.lse + (int64_t)b * T;
  int* st = w.state + (int64_t)b * T;
  float* fx = w.fx + (int64_t)b * T;
  const u64* bp64 = w.bp + (int64_t)b * T * w.nw;
  bp_t* bps = (bp_t*)bp64;
  const int64_t row_stride = w.nw * (8 / (int64_t)sizeof(bp_t));
  const int s0 = tid * K;
  // the thread's odd states s0 + 2 h + 1 carry labels; its even states s0 + 2 h are blanks
  int li[H];
  unsigned skipm = 0, freem = 0;
#pragma unroll
  for (int h = 0; h < H; ++h) {
    const int s = s0 + 2 * h + 1;
    const bool in = s < S;
    li[h] = in ? lab[s >> 1] : 0;
    if (in && s >= 3 && lab[s >> 1] != lab[(s >> 1) - 1]) skipm |= 1u << h;
    if (free_ends && (s - 1 == 0 || s - 1 == S - 1)) freem |= 1u << h;
  }
  // emissions of frames t, t + 1, t + 2 (raw logit; the frame's lse is subtracted where it is used); [H]: the blank
  float z0[H + 1], z1[H + 1], z2[H + 1];
  float l0 = lse[0], l1 = len > 1 ? lse[1] : 0.f, l2 = 0.f;
#pragma unroll
  for (int h = 0; h <= H; ++h) {
    const int k = h < H ? li[h] : 0;
    z0[h] = zb[k];
    z1[h] = len > 1 ? zb[ld + k] : 0.f;
    z2[h] = 0.f;
  }
  float v[K];
#pragma unroll
  for (int j = 0; j < K; ++j) v[j] = -INFINITY;
  if (tid == 0) {
    v[0] = (freem & 1u) ? 0.f : z0[H] - l0;
    if (S > 1) v[1] = z0[0] - l0;
  }
  edge[0][tid + 1] = v[K - 1];
  __syncthreads();
  int p = 0;
  for (int t = 1; t < len; ++t) {
    if (t + 1 < len) {
      l2 = lse[t + 1];
      const float* zr = zb + (int64_t)(t + 1) * ld;
#pragma unroll
      for (int h = 0; h < H; ++h) z2[h] = zr[li[h]];
      z2[H] = zr[0];
    }
    const float left = edge[p][tid];                         // state s0 - 1 of the frame before
    const float eb = z1[H] - l1;
    unsigned bits = 0;
#pragma unroll
    for (int j = K - 1; j >= 0; --j) {                       // from the top down: v[j - 1], v[j - 2] are still the frame before's
      const int h = j >> 1;
      const float a0 = v[j], a1 = j > 0 ? v[j - 1] : left;
      float a2 = -INFINITY;
      if ((j & 1) && ((skipm >> h) & 1u)) a2 = j > 1 ? v[j - 2] : left;
      float best = a0;
      unsigned c = 0;
      if (a1 > best) { best = a1; c = 1; }
      if (a2 > best) { best = a2; c = 2; }
      const float em = (j & 1) ? z1[h] - l1 : (((freem >> h) & 1u) ? 0.f : eb);
      v[j] = best + em;
      bits |= c << (2 * j);
    }
    edge[p ^ 1][tid + 1] = v[K - 1];
    if (s0 < S) bps[(int64_t)t * row_stride + tid] = (bp_t)bits;
    __syncthreads();
    p ^= 1;
    l1 = l2;
#pragma unroll
    for (int h = 0; h <= H; ++h) z1[h] = z2[h];
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if (s0 + j == S - 1) endv[0] = v[j];
    if (s0 + j == S - 2) endv[1] = v[j];
  }
  __syncthreads();
  // the backtrace (one wave): S - 1 unless S - 2 is strictly greater, then the stored choices down to frame 0
  if (tid < 64) {
    const float e1 = endv[0], e2 = endv[1];
    const float best = e2 > e1 ? e2 : e1;
    const int ok = best > -INFINITY;
    if (lane == 0) {
      feasible = ok;
      o.score[b] = ok ? best : -INFINITY;
    }
    if (ok) {
      int s = __builtin_amdgcn_readfirstlane(e2 > e1 ? S - 2 : S - 1);
      int t = len - 1;
      while (t >= 1) {
        const int n = t < 32 ? t : 32;                       // frames t, t - 1, ..., t - n + 1 (all >= 1)
        const int f = lane >> 1, W = s >> 5, w0 = W - 2 * (lane & 1);
        u64 a0 = 0, a1 = 0;
        if (f < n) {
          const u64* row = bp64 + (int64_t)(t - f) * w.nw;
          if (w0 >= 0) a0 = row[w0];
          if (w0 >= 1) a1 = row[w0 - 1];
        }
        int mine = 0;
        for (int i = 0; i < n; ++i) {
          if (lane == i) mine = s;
          const int d = W - (s >> 5);                        // 0 .. 2: the state fell by at most 2 i <= 62
          const u64 sel = (d & 1) ? a1 : a0;
          const int src = 2 * i + (d >> 1);
          const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)sel, src);
          const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(sel >> 32), src);
          const u64 word = ((u64)hi << 32) | lo;
          s -= (int)((word >> (2 * (s & 31))) & 3ull);
        }
        if (lane < n) st[t - lane] = mine;
        t -= n;
      }
      if (lane == 0) st[0] = s;
    }
  }
  __syncthreads();
  if (!feasible) {
    seg_infeasible(o, b, T, o0, L, u0, u1);
    return;
  }
  // the token of every frame and its log-probability; the frame where a label's run starts / ends (each label has exactly
  // one of either)
  for (int t = tid; t < T; t += nt) {
    if (t >= len) {
      pathb[t] = -1;
      continue;
    }
    const int s = st[t];
    const int tok = (s & 1) ? lab[s >> 1] : 0;
    pathb[t] = (free_ends && (s == 0 || s == S - 1)) ? -2 : tok;
    fx[t] = zb[(int64_t)t * ld + tok] - lse[t];
    if (s & 1) {
      if (t == 0 || st[t - 1] != s) o.first[o0 + (s >> 1)] = t;
      if (t == len - 1 || st[t + 1] != s) o.last[o0 + (s >> 1)] = t;
    }
  }
  __syncthreads();
  for (int i = tid; i < L; i += nt) {
    const int f = o.first[o0 + i], l = o.last[o0 + i], k = lab[i];
    float sum = 0.f;
    for (int t = f < 0 ? 0 : f; t <= l && t < len; ++t) sum += zb[(int64_t)t * ld + k] - lse[t];    // (0 <= f <= l < len)
    o.token_logp[o0 + i] = sum;
  }
  // the utterances: their label ranges tile [o0, o0 + L) (the host layer's check)
  for (int u = u0 + tid; u < u1; u += nt) {
    const int a = utt_offs[u], e = utt_offs[u + 1];
    if (e <= a || a < o0 || e > o0 + L) {
      o.utt_begin[u] = -1;
      o.utt_end[u] = -1;
      o.utt_logp[u] = 0.f;
      o.utt_conf[u] = 0.f;
      continue;
    }
    int bg = o.first[a], en = o.last[e - 1];
    bg = bg < 0 ? 0 : bg;
    en = en >= len ? len - 1 : en;                           // (0 <= bg <= en < len)
    float sum = 0.f, conf = INFINITY;
    for (int t = bg; t <= en; ++t) sum += fx[t];
    for (int t0 = bg; t0 <= en;) {
      const int n = en - t0 + 1 < window ? en - t0 + 1 : window;
      float blk = 0.f;
      for (int t = t0; t < t0 + n; ++t) blk += fx[t];
      const float mean = __fdiv_rn(blk, (float)n);
      conf = mean < conf ? mean : conf;
      t0 += n;
    }
    o.utt_begin[u] = bg;
    o.utt_end[u] = en;
    o.utt_logp[u] = sum;
    o.utt_conf[u] = conf;
  }
}

// the sizes a segmentation covers
inline int seg_shape_check(int B, int T, int V, int Lmax) {
  if (B <= 0 || T <= 0 || V <= 0 || Lmax < 0) return ASR_E_ARG;
  if (V < 2 || Lmax > kSegMaxL || ((int64_t)B * T + kLseWaves - 1) / kLseWaves > 0x7fffffffLL) return ASR_E_SHAPE;
  return 0;
}

}  // namespace

extern "C" int asr_ctc_segment_ws_bytes(int B, int T, int V, int max_label_len, int64_t* ws_bytes) {
  if (!ws_bytes) return ASR_E_ARG;
  const int rc = seg_shape_check(B, T, V, max_label_len);
  if (rc) return rc;
  *ws_bytes = seg_ws(nullptr, B, T, max_label_len).bytes;
  return 0;
}

extern "C" int asr_ctc_segment_f32(int B, int T, int V, const float* logits, int64_t ld, const int32_t* frame_lens,
                                   const int64_t* labels, const int32_t* label_offsets, int max_label_len, int free_ends, int N,
                                   const int32_t* utt_offsets, const int32_t* rec_utts, int window, int32_t* path, float* score,
                                   int32_t* first, int32_t* last, float* token_logp, int32_t* utt_begin, int32_t* utt_end,
                                   float* utt_logp, float* utt_conf, void* ws, int64_t ws_bytes, asr_stream_t stream) {
  if (!logits || !frame_lens || !label_offsets || !path || !score || !ws || ld < V) return ASR_E_ARG;
  if (max_label_len > 0 && (!labels || !first || !last || !token_logp)) return ASR_E_ARG;
  if (N < 0 || window < 1 || !utt_offsets || !rec_utts) return ASR_E_ARG;
  if (N > 0 && (!utt_begin || !utt_end || !utt_logp || !utt_conf)) return ASR_E_ARG;
  const int rc = seg_shape_check(B, T, V, max_label_len);
  if (rc) return rc;
  if ((((uintptr_t)ws) & 7u) != 0) return ASR_E_ALIGN;
  const SegWs w = seg_ws(ws, B, T, max_label_len);
  if (ws_bytes < w.bytes) return ASR_E_ARG;
  launch_frame_lse(B, T, V, logits, ld, frame_lens, w.lse, (hipStream_t)stream);
  ASR_CHECK_LAUNCH();
  const SegOut o = {path, score, first, last, token_logp, utt_begin, utt_end, utt_logp, utt_conf};
  const int Sp = 2 * max_label_len + 1;
  if (Sp <= kSegSmallStates) {
    const int nt = ((Sp + 3) / 4 + 63) / 64 * 64;
    hipLaunchKernelGGL(ctc_segment_kernel<4>, dim3(B), dim3(nt), 0, (hipStream_t)stream, T, V, logits, ld, frame_lens, labels,
                       label_offsets, max_label_len, free_ends, utt_offsets, rec_utts, window, o, w);
  } else {
    const int nt = ((Sp + 15) / 16 + 63) / 64 * 64;
    hipLaunchKernelGGL(ctc_segment_kernel<16>, dim3(B), dim3(nt), 0, (hipStream_t)stream, T, V, logits, ld, frame_lens, labels,
                       label_offsets, max_label_len, free_ends, utt_offsets, rec_utts, window, o, w);
  }
  ASR_CHECK_LAUNCH();
  return 0;
}
