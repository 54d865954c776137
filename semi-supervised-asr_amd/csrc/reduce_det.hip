// reduce_det.hip — ordered reductions: the deterministic counterparts of every fp32 atomicAdd on the train step's path
// (include/asr_hip.h, "Deterministic mode").
// One rule throughout: a result is a function of the inputs and the shapes only.  Partial sums are written with PLAIN stores
// into a caller-owned workspace by the workgroup that owns them, and a second launch adds them in index order; the launch
// boundary is the only synchronisation (no tickets, no fences, no float atomics in global memory or LDS).  Every sum below
// states its order; none of them is left to the compiler to re-associate (the adds across slabs / partials are __fadd_rn).
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ column sums
// Order of asr_colsum_det_f32.  Rows are cut into chunks of CH rows (CH = 256 on the float4 path, 512 on the scalar path).
//   inside a chunk, column n:  lane sums  l_r = X[m0 + r][n] + X[m0 + r + G][n] + ...  (ascending rows, G = 16 / 4 row groups),
//                              chunk sum  p = (((l_0 + l_1) + l_2) + ... + l_{G-1})      (float4 path: G = 16, in that order)
//                                         p = (l_0 + l_1) + (l_2 + l_3)                  (scalar path: G = 4)
//   over the chunks:           t = ((p_0 + p_1) + p_2) + ...                             (ascending chunk index)
//   out[n] = t, or out[n] + t with accumulate.
// One chunk: the first kernel writes out itself and no workspace is touched.
template <bool DIRECT>
__global__ void colsum_det_kernel(int64_t M, int64_t N, const float* __restrict__ X, int64_t ldx, float* __restrict__ dst,
                                  int accumulate) {
  __shared__ float part[4][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int64_t n = (int64_t)blockIdx.x * 64 + cx;
  const int64_t mbeg = (int64_t)blockIdx.y * 512;
  const int64_t mend = mbeg + 512 < M ? mbeg + 512 : M;
  float s = 0.f;
  if (n < N)
    for (int64_t m = mbeg + ry; m < mend; m += 4) s = __fadd_rn(s, X[m * ldx + n]);
  part[ry][cx] = s;
  __syncthreads();
  if (ry == 0 && n < N) {
    const float t = __fadd_rn(__fadd_rn(part[0][cx], part[1][cx]), __fadd_rn(part[2][cx], part[3][cx]));
    if (DIRECT) dst[n] = accumulate ? __fadd_rn(dst[n], t) : t;
    else dst[(int64_t)blockIdx.y * N + n] = t;
  }
}

template <bool DIRECT>
__global__ __launch_bounds__(256) void colsum4_det_kernel(int64_t M, int64_t N, const float* __restrict__ X, int64_t ldx,
                                                          float* __restrict__ dst, int accumulate) {
  __shared__ float4 part[16][16];
  const int cq = threadIdx.x & 15, ry = threadIdx.x >> 4;
  const int64_t n = (int64_t)blockIdx.x * 64 + 4 * cq;
  const int64_t mbeg = (int64_t)blockIdx.y * 256;
  const int64_t mend = mbeg + 256 < M ? mbeg + 256 : M;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (n < N) {
    const float* p = X + n;
#pragma unroll 4
    for (int64_t m = mbeg + ry; m < mend; m += 16) {
      const float4 v = *reinterpret_cast<const float4*>(p + m * ldx);
      s.x = __fadd_rn(s.x, v.x); s.y = __fadd_rn(s.y, v.y); s.z = __fadd_rn(s.z, v.z); s.w = __fadd_rn(s.w, v.w);
    }
  }
  part[ry][cq] = s;
  __syncthreads();
  if (threadIdx.x < 64) {
    const int q = threadIdx.x >> 2, e = threadIdx.x & 3;
    float t = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) t = __fadd_rn(t, reinterpret_cast<const float*>(&part[r][q])[e]);
    const int64_t col = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (col < N) {
      if (DIRECT) dst[col] = accumulate ? __fadd_rn(dst[col], t) : t;
      else dst[(int64_t)blockIdx.y * N + col] = t;
    }
  }
}

// out[n] = (accumulate ? out[n] : 0) + ((p_0[n] + p_1[n]) + ...): one owner per column, ascending partial index
__global__ void rows_combine_kernel(int64_t nparts, int64_t N, const float* __restrict__ parts, float* __restrict__ out,
                                    int accumulate, const float* __restrict__ gate) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  if (gate && !(gate[n] > 0.f)) return;
  float t = parts[n];
  for (int64_t k = 1; k < nparts; ++k) t = __fadd_rn(t, parts[k * N + n]);
  out[n] = accumulate ? __fadd_rn(out[n], t) : t;
}

// ------------------------------------------------------------------------------------------------ split-K combine
// C[m][n] = (((ws[0][m][n] + ws[1][m][n]) + ...) + ws[S-1][m][n]) (+ bias[n]) (+ C[m][n] if accumulate) (relu), each step
// one rounded fp32 add in exactly that order - bias, accumulate, relu as the epilogue of the unsplit asr_gemm_f32 applies
// them, so that S = 1 and S > 1 are the same function; ws slabs are dense [M][N].
__global__ __launch_bounds__(256) void gemm_det_combine_kernel(int64_t M, int64_t N, int S, const float* __restrict__ ws,
                                                               float* __restrict__ C, int64_t ldc,
                                                               const float* __restrict__ bias, int relu, int accumulate) {
  const int64_t MN = M * N;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < MN; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = i / N, n = i - m * N;
    float t = ws[i];
    for (int s = 1; s < S; ++s) t = __fadd_rn(t, ws[(int64_t)s * MN + i]);
    if (bias) t = __fadd_rn(t, bias[n]);
    float* c = C + m * ldc + n;
    if (accumulate) t = __fadd_rn(t, *c);
    if (relu) t = fmaxf(t, 0.f);
    *c = t;
  }
}

// ------------------------------------------------------------------------------------------------ embedding gradient
// One owner per (token id v, column quad): a = 0; for r = 0 .. rows-1 in order: if tokens[r] == v: a += grad[r]; then
// demb[v] = demb[v] + a.  Rows with a token outside [0, V) (-1: a step that was not fed a token) belong to nobody.
__global__ __launch_bounds__(256) void embedding_grad_det_kernel(int64_t rows, int E4, int V, const long long* __restrict__ tok,
                                                                 const float* __restrict__ grad, int64_t ldg,
                                                                 float* __restrict__ demb) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)V * E4) return;
  const long long v = i / E4;
  const int c = (int)(i - v * E4);
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  bool any = false;
  for (int64_t r = 0; r < rows; ++r) {
    if (tok[r] != v) continue;
    const float4 g = *reinterpret_cast<const float4*>(grad + r * ldg + 4 * c);
    a.x = __fadd_rn(a.x, g.x); a.y = __fadd_rn(a.y, g.y); a.z = __fadd_rn(a.z, g.z); a.w = __fadd_rn(a.w, g.w);
    any = true;
  }
  if (!any) return;
  float4* d = reinterpret_cast<float4*>(demb) + i;
  float4 o = *d;
  o.x = __fadd_rn(o.x, a.x); o.y = __fadd_rn(o.y, a.y); o.z = __fadd_rn(o.z, a.z); o.w = __fadd_rn(o.w, a.w);
  *d = o;
}

// ------------------------------------------------------------------------------------------------ pad-fill gradient
__device__ __forceinline__ float4 pad_mask_det(const float4* mask, int64_t i4, unsigned long long seed, unsigned thresh,
                                               float scale) {
  if (mask) return mask[i4];
  if (!thresh) return make_float4(1.f, 1.f, 1.f, 1.f);
  return make_float4(asr_drop_keep(seed, 4 * i4, thresh) ? scale : 0.f, asr_drop_keep(seed, 4 * i4 + 1, thresh) ? scale : 0.f,
                     asr_drop_keep(seed, 4 * i4 + 2, thresh) ? scale : 0.f, asr_drop_keep(seed, 4 * i4 + 3, thresh) ? scale : 0.f);
}

// part[b][c] = sum over the padded frames of utterance b of dout * mask: frame lane f sums the frames len + f, + FL, ... in
// ascending order, the lanes are added (((l_0 + l_1) + l_2) + ...); an utterance without padded frames stores zeros.  The
// second launch (rows_combine_kernel) adds the utterances in ascending b and applies the relu_of gate.
__global__ __launch_bounds__(512) void rows_fill_grad_det_kernel(int T, int C4, int FL, const float4* __restrict__ dout,
                                                                 const int32_t* __restrict__ lens,
                                                                 const float4* __restrict__ mask, unsigned long long seed,
                                                                 unsigned thresh, float scale, float4* __restrict__ part) {
  extern __shared__ float4 fold[];                         // [FL][C4]
  const int b = blockIdx.x;
  const int len = lens[b];
  const int c = threadIdx.x % C4, f = threadIdx.x / C4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (f < FL) {
    for (int t = (len < 0 ? 0 : len) + f; t < T; t += FL) {
      const int64_t o = ((int64_t)b * T + t) * C4 + c;
      const float4 g = dout[o], m = pad_mask_det(mask, o, seed, thresh, scale);
      acc.x = __fadd_rn(acc.x, __fmul_rn(g.x, m.x)); acc.y = __fadd_rn(acc.y, __fmul_rn(g.y, m.y));
      acc.z = __fadd_rn(acc.z, __fmul_rn(g.z, m.z)); acc.w = __fadd_rn(acc.w, __fmul_rn(g.w, m.w));
    }
    fold[f * C4 + c] = acc;
  }
  __syncthreads();
  if (f == 0) {
    for (int k = 1; k < FL; ++k) {
      const float4 v = fold[k * C4 + c];
      acc.x = __fadd_rn(acc.x, v.x); acc.y = __fadd_rn(acc.y, v.y); acc.z = __fadd_rn(acc.z, v.z); acc.w = __fadd_rn(acc.w, v.w);
    }
    part[(int64_t)b * C4 + c] = acc;
  }
}

// ------------------------------------------------------------------------------------------------ scalar sums
// Block sum in a fixed order: the lanes of a wave by the xor butterfly of wave_sum (offsets 32, 16, .. 1), then the four
// waves as (w_0 + w_1) + (w_2 + w_3).  Thread 0 returns the total.
__device__ __forceinline__ float block_sum_256(float s, float* part) {
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  return __fadd_rn(__fadd_rn(part[0], part[1]), __fadd_rn(part[2], part[3]));
}

// part[block] = sum of g^2 over the float4s block, block + grid, ... of thread-strided elements (the grid is a function of
// n alone); block 0 thread 0 also takes the n % 4 tail
__global__ __launch_bounds__(256) void sumsq_det_kernel(int64_t n4, int64_t n, const float* __restrict__ g,
                                                        float* __restrict__ part) {
  float s = 0.f;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = g4[i];
    s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t i = n4 * 4; i < n; ++i) s += g[i] * g[i];
  __shared__ float red[4];
  const float t = block_sum_256(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// out[0] = out[0] + scale * sum_i x[i]: ONE workgroup; thread t sums x[t], x[t + 256], ... in ascending order, then the
// block sum above.  Combines the partials of the sum-of-squares kernels (scale 1) and sums the loss rows (scale = the
// loss's constant).
__global__ __launch_bounds__(256) void sum_ordered_kernel(int64_t n, const float* __restrict__ x, float scale,
                                                          float* __restrict__ out) {
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += 256) s = __fadd_rn(s, x[i]);
  __shared__ float red[4];
  const float t = block_sum_256(s, red);
  if (threadIdx.x == 0) out[0] = __fadd_rn(out[0], __fmul_rn(scale, t));
}

// The gather of asr_gather_sumsq_f32 (csrc/optim.hip: same jobs, same chunks, same copies) with the block's sum of squares
// stored to part[block] instead of added to a word.
constexpr int GATHER_JOBS = ASR_GATHER_MAX_JOBS, GATHER_U = 8, GATHER_CHUNK = 256 * 4 * GATHER_U;
struct GatherJobsDet {
  int n;
  int first[GATHER_JOBS + 1];
  const float* src[GATHER_JOBS];
  int64_t dst[GATHER_JOBS];
  int64_t count[GATHER_JOBS];
};
__global__ __launch_bounds__(256) void gather_sumsq_det_kernel(GatherJobsDet t, float* __restrict__ flat,
                                                               float* __restrict__ part) {
  int lo = 0, hi = t.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t.first[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const int j = lo;
  const int64_t e0 = (int64_t)(blockIdx.x - t.first[j]) * GATHER_CHUNK;
  const int64_t e1 = e0 + GATHER_CHUNK < t.count[j] ? e0 + GATHER_CHUNK : t.count[j];
  const float* __restrict__ s = t.src[j];
  float* __restrict__ d = flat + t.dst[j];
  float acc = 0.f;
  if ((((uintptr_t)s) & 15) == 0 && (t.dst[j] & 3) == 0 && e1 - e0 == GATHER_CHUNK) {
    const float4* s4 = reinterpret_cast<const float4*>(s + e0);
    float4* d4 = reinterpret_cast<float4*>(d + e0);
    float4 v[GATHER_U];
#pragma unroll
    for (int u = 0; u < GATHER_U; ++u) v[u] = s4[threadIdx.x + 256 * u];
#pragma unroll
    for (int u = 0; u < GATHER_U; ++u) {
      d4[threadIdx.x + 256 * u] = v[u];
      acc += v[u].x * v[u].x + v[u].y * v[u].y + v[u].z * v[u].z + v[u].w * v[u].w;
    }
  } else if ((((uintptr_t)s) & 15) == 0 && (t.dst[j] & 3) == 0) {
    const int64_t n4 = (e1 - e0) >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(s + e0);
    float4* d4 = reinterpret_cast<float4*>(d + e0);
    for (int64_t i = threadIdx.x; i < n4; i += 256) {
      const float4 v = s4[i];
      d4[i] = v;
      acc += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    for (int64_t i = e0 + 4 * n4 + threadIdx.x; i < e1; i += 256) { const float v = s[i]; d[i] = v; acc += v * v; }
  } else {
    for (int64_t i = e0 + threadIdx.x; i < e1; i += 256) { const float v = s[i]; d[i] = v; acc += v * v; }
  }
  if (part) {
    __shared__ float red[4];
    const float tot = block_sum_256(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
  }
}

// K ranges of the deterministic split: `want` ranges asked for -> (ranges that exist, their length).  A range is
// ceil(K / want) long, rounded up to a multiple of 32 when that is at least 32 (the K step of the product kernels' tiles: every
// slab but the last then starts where the unsplit product would start a tile); the last range takes what is left.
void det_ranges(int64_t K, int64_t want, int* S, int64_t* kper) {
  if (want > K) want = K;
  if (want < 1) want = 1;
  int64_t kp = (K + want - 1) / want;
  if (kp >= 32) kp = (kp + 31) / 32 * 32;
  *kper = kp;
  *S = (int)((K + kp - 1) / kp);
}

// The split asr_gemm_det_f32 chooses when the caller names none: a function of M, N, K alone.  128 x 128 output tiles; a
// product whose tiles already fill the 256 CUs, or whose K is below 1 024, is not split; otherwise as many K ranges as bring
// the tiles to about one per CU, at most 16, each at least 512 long.
int64_t det_rule(int64_t M, int64_t N, int64_t K) {
  const int64_t tiles = ((M + 127) / 128) * ((N + 127) / 128);
  if (K < 1024 || tiles >= 256) return 1;
  int64_t s = 256 / tiles;
  if (s > 16) s = 16;
  if (s > K / 512) s = K / 512;
  return s < 1 ? 1 : s;
}

}  // namespace

extern "C" int asr_colsum_det_f32(int64_t M, int64_t N, const float* X, int64_t ldx, float* out, int accumulate, float* ws,
                                  int64_t ws_bytes, asr_stream_t stream_) {
  if (!X || !out || M <= 0 || N <= 0) return ASR_E_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  const bool vec = N % 4 == 0 && ldx % 4 == 0 && asr_aligned16(X);
  const int64_t ch = vec ? 256 : 512, chunks = (M + ch - 1) / ch;
  if (chunks > 65535) return ASR_E_SHAPE;
  const dim3 grid((unsigned)((N + 63) / 64), (unsigned)chunks);
  if (chunks == 1) {
    if (vec) hipLaunchKernelGGL((colsum4_det_kernel<true>), grid, dim3(256), 0, stream, M, N, X, ldx, out, accumulate);
    else hipLaunchKernelGGL((colsum_det_kernel<true>), grid, dim3(256), 0, stream, M, N, X, ldx, out, accumulate);
    ASR_CHECK_LAUNCH();
    return 0;
  }
  if (!ws || ws_bytes < chunks * N * (int64_t)sizeof(float)) return ASR_E_ARG;
  if (vec) hipLaunchKernelGGL((colsum4_det_kernel<false>), grid, dim3(256), 0, stream, M, N, X, ldx, ws, 0);
  else hipLaunchKernelGGL((colsum_det_kernel<false>), grid, dim3(256), 0, stream, M, N, X, ldx, ws, 0);
  hipLaunchKernelGGL(rows_combine_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, chunks, N, ws, out,
                     accumulate, (const float*)nullptr);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_gemm_det_ws_bytes(int transA, int transB, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                                     const float* B, int64_t ldb, const float* C, int64_t ldc, const float* bias, int relu,
                                     int accumulate, int batch, int64_t sA, int64_t sB, int64_t sC, int split_k, int arith,
                                     int64_t* ws_bytes, int* split, int64_t* k_range) {
  if (!ws_bytes) return ASR_E_ARG;
  *ws_bytes = 0;
  if (split) *split = 1;
  if (k_range) *k_range = K;
  asr_gemm_plan_t plan;
  // the refusals of the call that will run: the unsplit product when there is one range, a batch of slabs otherwise
  int rc = asr_gemm_plan(transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, relu, accumulate, batch, sA, sB, sC, 1,
                         arith & ~ASR_GEMM_C_ZEROED, 0, &plan);
  if (rc) return rc;
  int S;
  int64_t kper;
  det_ranges(K, split_k >= 1 ? (int64_t)split_k : det_rule(M, N, K), &S, &kper);
  if (S == 1) return 0;
  const int64_t stepA = kper * (transA ? lda : 1), stepB = kper * (transB ? 1 : ldb);
  rc = asr_gemm_plan(transA, transB, M, N, kper, A, lda, B, ldb, C, N, nullptr, 0, 0, (int)(K / kper), stepA, stepB, M * N, 1,
                     arith & ~ASR_GEMM_C_ZEROED, 0, &plan);
  if (rc) return rc;
  const int64_t rem = K - (K / kper) * kper;       // ... and the shorter last range, a launch of its own
  if (rem > 0) {
    rc = asr_gemm_plan(transA, transB, M, N, rem, A + (K / kper) * stepA, lda, B + (K / kper) * stepB, ldb, C, N, nullptr, 0, 0, 1,
                       0, 0, 0, 1, arith & ~ASR_GEMM_C_ZEROED, 0, &plan);
    if (rc) return rc;
  }
  *ws_bytes = (int64_t)S * M * N * (int64_t)sizeof(float);
  if (split) *split = S;
  if (k_range) *k_range = kper;
  return 0;
}

extern "C" int asr_gemm_det_f32(int transA, int transB, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                                const float* B, int64_t ldb, float* C, int64_t ldc, const float* bias, int relu,
                                int accumulate, int batch, int64_t sA, int64_t sB, int64_t sC, int split_k, int arith,
                                float* ws, int64_t ws_bytes, asr_stream_t stream) {
  int64_t need, kper;
  int S;
  int rc = asr_gemm_det_ws_bytes(transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, relu, accumulate, batch, sA, sB, sC,
                                 split_k, arith, &need, &S, &kper);
  if (rc) return rc;
  arith &= ~ASR_GEMM_C_ZEROED;
  if (S == 1)
    return asr_gemm_f32(transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, relu, accumulate, batch, sA, sB, sC, 1, arith,
                        stream);
  if (!ws || ws_bytes < need || !asr_aligned16(ws)) return ASR_E_ARG;
  const int64_t stepA = kper * (transA ? lda : 1), stepB = kper * (transB ? 1 : ldb), MN = M * N;
  const int nfull = (int)(K / kper);
  const int64_t rem = K - (int64_t)nfull * kper;
  const int64_t blocks = (MN + 255) / 256;
  for (int b = 0; b < batch; ++b) {          // (the products of a batch share the workspace: they are stream-ordered)
    const float* Ab = A + (int64_t)b * sA;
    const float* Bb = B + (int64_t)b * sB;
    rc = asr_gemm_f32(transA, transB, M, N, kper, Ab, lda, Bb, ldb, ws, N, nullptr, 0, 0, nfull, stepA, stepB, MN, 1, arith,
                      stream);
    if (rc) return rc;
    if (rem > 0) {
      rc = asr_gemm_f32(transA, transB, M, N, rem, Ab + nfull * stepA, lda, Bb + nfull * stepB, ldb, ws + (int64_t)nfull * MN, N,
                        nullptr, 0, 0, 1, 0, 0, 0, 1, arith, stream);
      if (rc) return rc;
    }
    hipLaunchKernelGGL(gemm_det_combine_kernel, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0,
                       (hipStream_t)stream, M, N, S, ws, C + (int64_t)b * sC, ldc, bias, relu, accumulate);
  }
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_embedding_grad_det_f32(int64_t rows, int E, int V, const long long* tokens, const float* grad, int64_t ldg,
                                          float* demb, asr_stream_t stream) {
  if (rows <= 0 || E <= 0 || V <= 0 || !tokens || !grad || !demb) return ASR_E_ARG;
  if (E % 4 || ldg % 4 || (int64_t)V * E * 4 > 65536) return ASR_E_SHAPE;
  if (!asr_aligned16(grad) || !asr_aligned16(demb)) return ASR_E_ALIGN;
  const int64_t n = (int64_t)V * (E / 4);
  hipLaunchKernelGGL(embedding_grad_det_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rows, E / 4,
                     V, tokens, grad, ldg, demb);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_rows_fill_grad_det_f32(int B, int T, int C, const float* dout, const int32_t* lens, const float* mask,
                                          uint64_t seed, float p, float* dfill, const float* relu_of, float* ws,
                                          int64_t ws_bytes, asr_stream_t stream) {
  if (!dout || !lens || !dfill || B <= 0 || T <= 0 || C <= 0 || p < 0.f || p >= 1.f) return ASR_E_ARG;
  if (C % 4 || C / 4 > 512) return ASR_E_SHAPE;
  if (!ws || ws_bytes < (int64_t)B * C * (int64_t)sizeof(float)) return ASR_E_ARG;
  if (!asr_aligned16(dout) || !asr_aligned16(ws) || (mask && !asr_aligned16(mask))) return ASR_E_ALIGN;
  const int C4 = C / 4;
  int FL = 512 / C4;
  if (FL > 8) FL = 8;
  hipLaunchKernelGGL(rows_fill_grad_det_kernel, dim3(B), dim3(FL * C4), (size_t)FL * C4 * sizeof(float4), (hipStream_t)stream, T,
                     C4, FL, (const float4*)dout, lens, (const float4*)mask, seed, mask ? 0u : asr_drop_thresh(p),
                     1.0f / (1.0f - p), (float4*)ws);
  hipLaunchKernelGGL(rows_combine_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int64_t)B,
                     (int64_t)C, ws, dfill, 1, relu_of);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_sum_det_f32(int64_t n, const float* x, float scale, float* out, asr_stream_t stream) {
  if (!x || !out || n <= 0) return ASR_E_ARG;
  hipLaunchKernelGGL(sum_ordered_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n, x, scale, out);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_sumsq_det_f32(int64_t n, const float* g, float* out, float* ws, int64_t ws_bytes, asr_stream_t stream) {
  if (!g || !out || n <= 0 || !ws || ws_bytes < ASR_SUMSQ_DET_WS_BYTES) return ASR_E_ARG;
  if (!asr_aligned16(g)) return ASR_E_ALIGN;
  const int64_t n4 = n / 4;
  int64_t nb = (n4 + 255) / 256;
  if (nb < 1) nb = 1;
  if (nb > 1024) nb = 1024;
  hipLaunchKernelGGL(sumsq_det_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, n4, n, g, ws);
  hipLaunchKernelGGL(sum_ordered_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nb, ws, 1.0f, out);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_gather_sumsq_det_f32(int njobs, const float* const* src, const int64_t* dst_offset, const int64_t* count,
                                        float* flat, float* sumsq, float* ws, int64_t ws_bytes, asr_stream_t stream) {
  if (njobs <= 0 || !src || !dst_offset || !count || !flat) return ASR_E_ARG;
  if (sumsq && !ws) return ASR_E_ARG;
  for (int j0 = 0; j0 < njobs; j0 += GATHER_JOBS) {
    GatherJobsDet t;
    t.n = njobs - j0 < GATHER_JOBS ? njobs - j0 : GATHER_JOBS;
    int64_t at = 0;
    for (int j = 0; j < GATHER_JOBS; ++j) {
      t.first[j] = (int)at;
      if (j < t.n) {
        if (!src[j0 + j] || count[j0 + j] <= 0 || dst_offset[j0 + j] < 0) return ASR_E_ARG;
        t.src[j] = src[j0 + j]; t.dst[j] = dst_offset[j0 + j]; t.count[j] = count[j0 + j];
        at += (count[j0 + j] + GATHER_CHUNK - 1) / GATHER_CHUNK;
        if (at > 0x7fffffff) return ASR_E_SHAPE;
      } else {
        t.src[j] = nullptr; t.dst[j] = 0; t.count[j] = 0;
      }
    }
    t.first[GATHER_JOBS] = (int)at;
    if (sumsq && ws_bytes < at * (int64_t)sizeof(float)) return ASR_E_ARG;
    hipLaunchKernelGGL(gather_sumsq_det_kernel, dim3((unsigned)at), dim3(256), 0, (hipStream_t)stream, t, flat,
                       sumsq ? ws : (float*)nullptr);
    // (the launches of a long job list share the workspace and add to the word in launch order: stream-ordered)
    if (sumsq) hipLaunchKernelGGL(sum_ordered_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, at, ws, 1.0f, sumsq);
  }
  ASR_CHECK_LAUNCH();
  return 0;
}
