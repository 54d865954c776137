// ctc_star.hip — star CTC: the CTC loss for transcripts with missing words, forward and backward.
// Between any two labels (and before the first, behind the last) the lattice may pass through a star state that emits "any
// non-blank token" at a price, penalty[b] <= 0 per frame.  The conventions are seq_common.h's (blank 0, x = z - lse, ordered
// sums); alpha / beta are kept in log space.  States of an utterance with labels l_1 .. l_L, S = 3 L + 2 of them:
//   s = 0: b_0   s = 1: s_0   then for g = 1 .. L   s = 3g - 1: l_g   s = 3g: b_g   s = 3g + 1: s_g
//   kind(s) = (s + 1) % 3: 0 label, 1 blank, 2 star;  g(s) = (s + 1) / 3
//   emission    b_g: x[t][0]   l_g: x[t][l_g]   s_g: nb[t] + penalty[b],  nb[t] = logsumexp_{v >= 1} z[t][v] - lse[t]
//   into b_g:   b_g (s), s_g (s + 1), l_g (s - 1)
//   into s_g:   s_g (s), b_g (s - 1), l_g (s - 2)
//   into l_g:   l_g (s), s_{g-1} (s - 1), b_{g-1} (s - 2), and l_{g-1} (s - 3) where g >= 2 and l_g != l_{g-1}
//   frame 0 sits in s < 3; the path ends in s >= S - 3 (for L = 0 both say: b_0 or s_0)
// penalty = -inf leaves the star states unreachable: the plain CTC lattice.
//   star_frame_kernel  one wave per frame: lse[t] and nb[t], both sums in one pass over the row (each a direct log-sum-exp)
//   star_alpha_kernel  one workgroup per utterance (one wave when max S <= 64): the label-sorted position list (once), then
//                      alpha over the frames - states across threads (strided when S exceeds the workgroup), the hand-off
//                      between frames through two rows of LDS with one barrier per frame, two frames of register prefetch
//   star_beta_kernel   the same chain backwards; writes the log occupancy of (t, s) over alpha_t(s)
//   star_grad_kernel   one wave per frame: the blank's and the star's states are summed by the whole wave, every other
//                      vocabulary entry by the lane that owns it, walking its run of the sorted position list in ascending order
#include "seq_common.h"

namespace {

constexpr int kStarMaxL = ASR_CTC_STAR_MAX_LABELS;
static_assert(3 * kStarMaxL + 2 <= kMaxS, "the star lattice must fit the LDS rows and launch_by_states of the CTC chains");
constexpr int kStarHeadShift = 12;             // head entry = (first index in the sorted list << 12) | run length; 0: absent
static_assert(kStarMaxL < (1 << kStarHeadShift), "the run length must fit the low bits of a head entry");

struct StarWs {
  float* lse;      // [B][T]
  float* nb;       // [B][T]         log of the non-blank share of the frame
  float* raw;      // [B]            the nll before zero_infinity
  float* ab;       // [B][T][Sp]     alpha; after the backward's first kernel the log occupancy of (t, s);  Sp = 3 max_label_len + 2
  int* order;      // [B][Lo]        label positions sorted by (label, position);  Lo = max(max_label_len, 1)
  int* head;       // [B][V]
  int64_t bytes;
};

StarWs star_ws(void* base, int B, int T, int V, int Lmax) {
  const int64_t Sp = 3 * (int64_t)Lmax + 2, Lo = Lmax > 0 ? Lmax : 1;
  const int64_t n_lse = round64((int64_t)B * T), n_raw = round64(B), n_ab = round64((int64_t)B * T * Sp),
                n_order = round64((int64_t)B * Lo), n_head = round64((int64_t)B * V);
  StarWs w;
  float* f = (float*)base;
  w.lse = f;
  w.nb = w.lse + n_lse;
  w.raw = w.nb + n_lse;
  w.ab = w.raw + n_raw;
  w.order = (int*)(w.ab + n_ab);
  w.head = w.order + n_order;
  w.bytes = 4 * (2 * n_lse + n_raw + n_ab + n_order + n_head);
  return w;
}

__device__ __forceinline__ float lse4(float a, float b, float c, float d) {
  const float m = fmaxf(fmaxf(a, b), fmaxf(c, d));
  if (m == -INFINITY) return -INFINITY;
  return m + logf(expf(a - m) + expf(b - m) + expf(c - m) + expf(d - m));
}

// one wave per valid frame: lse = logsumexp_v z (the bits of frame_lse_kernel) and nb = logsumexp_{v >= 1} z - lse, the
// second about its own maximum (never log(1 - p_0), which cancels when the blank owns the frame)
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void star_frame_kernel(int B, int T, int V, const float* __restrict__ z, int64_t ld,
                                                                const int32_t* __restrict__ lens, float* __restrict__ lse,
                                                                float* __restrict__ nb) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (row >= (int64_t)B * T) return;
  const int b = (int)(row / T), t = (int)(row % T);
  if (t >= lens[b]) return;                                 // frames behind the utterance are never read
  const float* zr = z + row * ld;
  float mn = -INFINITY;
  for (int v = lane; v < V; v += 64) mn = v > 0 ? fmaxf(mn, zr[v]) : mn;
  mn = wave_max(mn);
  const float mx = fmaxf(mn, zr[0]);
  float se = 0.f, sn = 0.f;
  for (int v = lane; v < V; v += 64) {
    const float x = zr[v];
    se += expf(x - mx);
    if (v > 0 && mn > -INFINITY) sn += expf(x - mn);
  }
  se = wave_sum(se);
  sn = wave_sum(sn);
  if (lane == 0) {
    const float l = mx + logf(se);
    lse[row] = l;
    nb[row] = mn > -INFINITY ? (mn + logf(sn)) - l : -INFINITY;
  }
}

template <int NS>
__global__ __launch_bounds__(256) void star_alpha_kernel(int T, int V, const float* __restrict__ z, int64_t ld,
                                                         const int32_t* __restrict__ lens,
                                                         const int64_t* __restrict__ labels,
                                                         const int32_t* __restrict__ offs,
                                                         const float* __restrict__ penalty, int Lmax, int zero_inf,
                                                         float* __restrict__ nll, StarWs w) {
  __shared__ float buf[2][kMaxS + 5];          // alpha of the previous / this frame at [s + 3]; [0 .. 2] stay -inf
  __shared__ int lab[kMaxL + 1];
  __shared__ int bad;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int o0 = offs[b], L = offs[b + 1] - o0, S = 3 * L + 2;
  const int Sp = 3 * Lmax + 2, Lo = Lmax > 0 ? Lmax : 1;
  const int len = clamp_len(lens[b], T);
  for (int k = tid; k < V; k += nt) w.head[(int64_t)b * V + k] = 0;
  for (int i = tid; i < 2 * (kMaxS + 5); i += nt) (&buf[0][0])[i] = -INFINITY;
  const bool ok = ctc_load_labels(labels, o0, L, Lmax, V, lab, &bad);      // (its barriers order the fills above)
  if (!ok || len == 0) {                       // no frame: no path, whatever L
    if (tid == 0) {
      w.raw[b] = INFINITY;
      nll[b] = zero_inf ? 0.f : INFINITY;
    }
    return;
  }
  // the sorted position list, as ctc_alpha_kernel builds it
  for (int i = tid; i < L; i += nt) {
    const int li = lab[i];
    int less = 0, eq_before = 0, eq = 0;
    for (int j = 0; j < L; ++j) {
      const int lj = lab[j];
      less += lj < li;
      eq += lj == li;
      eq_before += (lj == li) & (j < i);
    }
    const int r = less + eq_before;
    w.order[(int64_t)b * Lo + r] = i;
    if (eq_before == 0) w.head[(int64_t)b * V + li] = (r << kStarHeadShift) | eq;
  }
  const float* zb = z + (int64_t)b * T * ld;
  const float* lse = w.lse + (int64_t)b * T;
  const float* nbr = w.nb + (int64_t)b * T;
  float* ab = w.ab + (int64_t)b * T * Sp;
  const float npen = -penalty[b];              // a star emission is nb - npen; npen = +inf: never
  int li[NS], third[NS];
  bool act[NS], star[NS], skip[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int s = tid + i * nt, kind = (s + 1) % 3, g = (s + 1) / 3;
    act[i] = s < S;
    star[i] = kind == 2;
    li[i] = (act[i] && kind == 0) ? lab[g - 1] : 0;
    skip[i] = act[i] && kind == 0 && g >= 2 && lab[g - 1] != lab[g - 2];
    third[i] = kind == 1 ? s + 4 : s + 1;      // the third predecessor's place in buf: s_g of a blank, s - 2 otherwise
  }
  // emissions of frames t, t + 1, t + 2 (raw logit or nb; the frame's lse / the penalty is subtracted where it is used)
  float z0[NS], z1[NS], z2[NS];
  float l0 = lse[0], l1 = len > 1 ? lse[1] : 0.f, l2 = 0.f;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    z0[i] = act[i] ? (star[i] ? nbr[0] : zb[li[i]]) : 0.f;
    z1[i] = (act[i] && len > 1) ? (star[i] ? nbr[1] : zb[ld + li[i]]) : 0.f;
    z2[i] = 0.f;
  }
  int p = 0;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int s = tid + i * nt;
    if (act[i]) {
      const float a = s < 3 ? z0[i] - (star[i] ? npen : l0) : -INFINITY;
      buf[0][s + 3] = a;
      ab[s] = a;
    }
  }
  __syncthreads();
  for (int t = 1; t < len; ++t) {
    if (t + 1 < len) {
      l2 = lse[t + 1];
#pragma unroll
      for (int i = 0; i < NS; ++i)
        if (act[i]) z2[i] = star[i] ? nbr[t + 1] : zb[(int64_t)(t + 1) * ld + li[i]];
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int s = tid + i * nt;
      if (act[i]) {
        const float a0 = buf[p][s + 3], a1 = buf[p][s + 2], a2 = buf[p][third[i]], a3 = skip[i] ? buf[p][s] : -INFINITY;
        const float a = lse4(a0, a1, a2, a3) + (z1[i] - (star[i] ? npen : l1));
        buf[p ^ 1][s + 3] = a;
        ab[(int64_t)t * Sp + s] = a;
      }
    }
    __syncthreads();
    p ^= 1;
    l1 = l2;
#pragma unroll
    for (int i = 0; i < NS; ++i) z1[i] = z2[i];
  }
  if (tid == 0) {
    const float r = -lse4(buf[p][S - 1 + 3], buf[p][S - 2 + 3], buf[p][S - 3 + 3], -INFINITY);   // (L = 0: [2] is -inf)
    w.raw[b] = r;
    nll[b] = (zero_inf && !(r < INFINITY)) ? 0.f : r;
  }
}

// beta_t(s) = emission_t(s) + logsum over the successors' beta_{t+1}; what goes over alpha_t(s) is alpha_t(s) + that logsum
// WITHOUT the emission (the log of the mass of the paths through (t, s), each emission counted once) + nll_b: the log of the
// state's occupancy (star_log_occupancy).
//   out of b_g:  b_g (s), s_g (s + 1), l_{g+1} (s + 2)
//   out of s_g:  s_g (s), b_g (s - 1), l_{g+1} (s + 1)
//   out of l_g:  l_g (s), b_g (s + 1), s_g (s + 2), and l_{g+1} (s + 3) where l_{g+1} != l_g
// alpha + out + nll.  alpha + out is about -nll, far larger than the log occupancy that is left of it, and its rounding (an
// ulp of nll) would be the gradient's error: the sum is taken exactly (two-sum: s and its rounding error e), s + nll cancels
// without rounding where the occupancy is not negligible, and e joins behind.
__device__ __forceinline__ float star_log_occupancy(float alpha, float out, float nll) {
  const float s = alpha + out;
  if (!(s > -INFINITY)) return -INFINITY;
  const float o = s - alpha;
  const float e = (alpha - (s - o)) + (out - o);
  return (s + nll) + e;
}

template <int NS>
__global__ __launch_bounds__(256) void star_beta_kernel(int T, int V, const float* __restrict__ z, int64_t ld,
                                                        const int32_t* __restrict__ lens,
                                                        const int64_t* __restrict__ labels,
                                                        const int32_t* __restrict__ offs,
                                                        const float* __restrict__ penalty, int Lmax, StarWs w) {
  __shared__ float buf[2][kMaxS + 5];          // beta of the next / this frame at [s + 1]; [0] and everything from [S + 1] on stay -inf
  __shared__ int lab[kMaxL + 1];
  __shared__ int bad;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const float nllb = w.raw[b];
  if (!(nllb < INFINITY)) return;              // infeasible: the gradient kernel does not read the occupancies
  const int o0 = offs[b], L = offs[b + 1] - o0, S = 3 * L + 2;
  const int Sp = 3 * Lmax + 2;
  const int len = clamp_len(lens[b], T);
  for (int i = tid; i < 2 * (kMaxS + 5); i += nt) (&buf[0][0])[i] = -INFINITY;
  if (!ctc_load_labels(labels, o0, L, Lmax, V, lab, &bad) || len == 0) return;
  const float* zb = z + (int64_t)b * T * ld;
  const float* lse = w.lse + (int64_t)b * T;
  const float* nbr = w.nb + (int64_t)b * T;
  float* ab = w.ab + (int64_t)b * T * Sp;
  const float npen = -penalty[b];
  int li[NS], third[NS];
  bool act[NS], star[NS], skip[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int s = tid + i * nt, kind = (s + 1) % 3, g = (s + 1) / 3;
    act[i] = s < S;
    star[i] = kind == 2;
    li[i] = (act[i] && kind == 0) ? lab[g - 1] : 0;
    skip[i] = act[i] && kind == 0 && g < L && lab[g - 1] != lab[g];
    third[i] = kind == 2 ? s : s + 3;          // the third successor's place in buf: b_g of a star, s + 2 otherwise
  }
  // emissions and alpha of frames t, t - 1, t - 2
  float z0[NS], z1[NS], z2[NS], a0[NS], a1[NS], a2[NS];
  int t = len - 1;
  float l0 = lse[t], l1 = t > 0 ? lse[t - 1] : 0.f, l2 = 0.f;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int s = tid + i * nt;
    z0[i] = act[i] ? (star[i] ? nbr[t] : zb[(int64_t)t * ld + li[i]]) : 0.f;
    a0[i] = act[i] ? ab[(int64_t)t * Sp + s] : 0.f;
    z1[i] = (act[i] && t > 0) ? (star[i] ? nbr[t - 1] : zb[(int64_t)(t - 1) * ld + li[i]]) : 0.f;
    a1[i] = (act[i] && t > 0) ? ab[(int64_t)(t - 1) * Sp + s] : 0.f;
    z2[i] = a2[i] = 0.f;
  }
  int p = 0;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int s = tid + i * nt;
    if (act[i]) {
      const float out = s >= S - 3 ? 0.f : -INFINITY;
      buf[0][s + 1] = out + (z0[i] - (star[i] ? npen : l0));
      ab[(int64_t)t * Sp + s] = star_log_occupancy(a0[i], out, nllb);
    }
  }
  __syncthreads();
  for (t = len - 2; t >= 0; --t) {
    if (t > 0) {
      l2 = lse[t - 1];
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const int s = tid + i * nt;
        if (act[i]) {
          z2[i] = star[i] ? nbr[t - 1] : zb[(int64_t)(t - 1) * ld + li[i]];
          a2[i] = ab[(int64_t)(t - 1) * Sp + s];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int s = tid + i * nt;
      if (act[i]) {
        const float b0 = buf[p][s + 1], b1 = buf[p][s + 2], b2 = buf[p][third[i]], b3 = skip[i] ? buf[p][s + 4] : -INFINITY;
        const float out = lse4(b0, b1, b2, b3);
        buf[p ^ 1][s + 1] = out + (z1[i] - (star[i] ? npen : l1));
        ab[(int64_t)t * Sp + s] = star_log_occupancy(a1[i], out, nllb);
      }
    }
    __syncthreads();
    p ^= 1;
    l1 = l2;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      z1[i] = z2[i];
      a1[i] = a2[i];
    }
  }
}

// the entries first, first + step, .. below n of one frame's log occupancies: lane-strided in ascending order, then the xor
// butterfly
__device__ __forceinline__ float star_wave_logsum(const float* abr, int first, int step, int n, int lane) {
  float m = -INFINITY;
  for (int s = first + lane * step; s < n; s += 64 * step) m = fmaxf(m, abr[s]);
  m = wave_max(m);
  if (!(m > -INFINITY)) return -INFINITY;                    // (wave-uniform)
  float se = 0.f;
  for (int s = first + lane * step; s < n; s += 64 * step) se += expf(abr[s] - m);
  return m + logf(wave_sum(se));
}

// dz[b][t][k] = g_b (softmax_k - occ_k), occ_k = exp(logsum_{s : label k} lg_t(s) - all_t)
//                                              + [k >= 1] exp(logsum_g lg_t(s_g) - all_t + x[t][k] - nb[t]);
// lg the log occupancies of star_beta_kernel and all_t = logsum_s lg_t(s), which is 0 up to rounding: the occupancies of a
// frame are normalised by the frame's own total, so what the chains' roundings have in common at frame t (|alpha| grows
// with t, and its ulp with it) cancels.  Zeros behind the utterance.
__global__ __launch_bounds__(256) void star_grad_kernel(int B, int T, int V, const float* __restrict__ z, int64_t ld,
                                                        const int32_t* __restrict__ lens,
                                                        const int32_t* __restrict__ offs, int Lmax, int zero_inf,
                                                        const float* __restrict__ g, StarWs w, float* __restrict__ dz,
                                                        int64_t lddz) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (int64_t)B * T) return;
  const int b = (int)(row / T), t = (int)(row % T);
  float* dzr = dz + row * lddz;
  const float nllb = w.raw[b];
  const bool feasible = nllb < INFINITY;
  if (t >= lens[b] || (!feasible && zero_inf)) {
    for (int k = lane; k < V; k += 64) dzr[k] = 0.f;
    return;
  }
  const float* zr = z + row * ld;
  const float ls = w.lse[row], gb = g[b];
  if (!feasible) {                                           // no alignment: only the softmax term is defined
    for (int k = lane; k < V; k += 64) dzr[k] = gb * expf(zr[k] - ls);
    return;
  }
  const int L = offs[b + 1] - offs[b];
  const int Sp = 3 * Lmax + 2, Lo = Lmax > 0 ? Lmax : 1;
  const float* abr = w.ab + row * Sp;
  const int* order = w.order + (int64_t)b * Lo;
  const int* head = w.head + (int64_t)b * V;
  const int S = 3 * L + 2;
  const float lall = star_wave_logsum(abr, 0, 1, S, lane);   // every state (finite: the row has a path, and it crosses frame t)
  const float lblank = star_wave_logsum(abr, 0, 3, S, lane); // b_0 .. b_L
  const float lstar = star_wave_logsum(abr, 1, 3, S, lane);  // s_0 .. s_L
  const float share = lstar > -INFINITY ? lstar - lall - w.nb[row] : -INFINITY;   // (nb is finite where a star has mass)
  for (int k = lane; k < V; k += 64) {
    const float lp = zr[k] - ls;
    float lsum = lblank;
    if (k > 0) {
      const int e = head[k], n = e & ((1 << kStarHeadShift) - 1), h = e >> kStarHeadShift;
      lsum = -INFINITY;
      if (n > 0) {
        float mk = -INFINITY;
        for (int j = 0; j < n; ++j) mk = fmaxf(mk, abr[3 * order[h + j] + 2]);
        if (mk > -INFINITY) {
          float se = 0.f;
          for (int j = 0; j < n; ++j) se += expf(abr[3 * order[h + j] + 2] - mk);
          lsum = mk + logf(se);
        }
      }
    }
    float occ = lsum > -INFINITY ? expf(lsum - lall) : 0.f;
    if (k > 0 && share > -INFINITY) occ += expf(share + lp);
    dzr[k] = gb * (expf(lp) - occ);
  }
}

int star_check(int B, int T, int V, int64_t ld, int Lmax, const void* ws, int64_t ws_bytes) {
  const int rc = ctc_shape_check(B, T, V, Lmax);
  if (rc == ASR_E_ARG || ld < V || !ws) return ASR_E_ARG;
  if (rc) return rc;
  if (Lmax > kStarMaxL) return ASR_E_SHAPE;
  if (((uintptr_t)ws & 3) || ws_bytes < star_ws(nullptr, B, T, V, Lmax).bytes) return ASR_E_ARG;
  return 0;
}

}  // namespace

extern "C" int asr_ctc_star_ws_bytes(int B, int T, int V, int max_label_len, int64_t* ws_bytes) {
  if (B <= 0 || T <= 0 || V <= 0 || max_label_len < 0 || !ws_bytes) return ASR_E_ARG;
  if (V < 2 || max_label_len > kStarMaxL) return ASR_E_SHAPE;
  *ws_bytes = star_ws(nullptr, B, T, V, max_label_len).bytes;
  return 0;
}

extern "C" int asr_ctc_star_loss_fwd(int B, int T, int V, const float* logits, int64_t ld, const int32_t* frame_lens,
                                     const int64_t* labels, const int32_t* label_offsets, int max_label_len,
                                     const float* penalty, int zero_infinity, float* nll, void* ws, int64_t ws_bytes,
                                     asr_stream_t stream) {
  if (!logits || !frame_lens || !labels || !label_offsets || !penalty || !nll) return ASR_E_ARG;
  const int rc = star_check(B, T, V, ld, max_label_len, ws, ws_bytes);
  if (rc) return rc;
  const StarWs w = star_ws(ws, B, T, V, max_label_len);
  const unsigned groups = (unsigned)(((int64_t)B * T + kLseWaves - 1) / kLseWaves);
  hipLaunchKernelGGL(star_frame_kernel<kLseWaves>, dim3(groups), dim3(64 * kLseWaves), 0, (hipStream_t)stream, B, T, V, logits,
                     ld, frame_lens, w.lse, w.nb);
  ASR_CHECK_LAUNCH();
  launch_by_states(3 * max_label_len + 2, star_alpha_kernel<1>, star_alpha_kernel<8>, B, (hipStream_t)stream, T, V, logits, ld,
                   frame_lens, labels, label_offsets, penalty, max_label_len, zero_infinity, nll, w);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_ctc_star_loss_bwd(int B, int T, int V, const float* logits, int64_t ld, const int32_t* frame_lens,
                                     const int64_t* labels, const int32_t* label_offsets, int max_label_len,
                                     const float* penalty, int zero_infinity, const float* grad_nll, void* ws,
                                     int64_t ws_bytes, float* dlogits, int64_t lddz, asr_stream_t stream) {
  if (!logits || !frame_lens || !labels || !label_offsets || !penalty || !grad_nll || !dlogits || lddz < V) return ASR_E_ARG;
  const int rc = star_check(B, T, V, ld, max_label_len, ws, ws_bytes);
  if (rc) return rc;
  const StarWs w = star_ws(ws, B, T, V, max_label_len);
  launch_by_states(3 * max_label_len + 2, star_beta_kernel<1>, star_beta_kernel<8>, B, (hipStream_t)stream, T, V, logits, ld,
                   frame_lens, labels, label_offsets, penalty, max_label_len, w);
  ASR_CHECK_LAUNCH();
  const unsigned rows4 = (unsigned)(((int64_t)B * T + 3) / 4);
  hipLaunchKernelGGL(star_grad_kernel, dim3(rows4), dim3(256), 0, (hipStream_t)stream, B, T, V, logits, ld, frame_lens,
                     label_offsets, max_label_len, zero_infinity, grad_nll, w, dlogits, lddz);
  ASR_CHECK_LAUNCH();
  return 0;
}
