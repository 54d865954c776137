// edit_distance.hip — batched Levenshtein distance on token ids (the scoring half of CER, utils.py:222-228 of the
// reference: editdistance.eval per utterance).  One wave per (hypothesis, reference) pair, one 64-thread
// workgroup per wave, so that 32 .. 512 pairs spread over the CUs.
//   phase 1  compaction into LDS: the hypothesis row is cut before its first <EOS>, both sides drop the tokens of the skip
//            table (ballot + popcount prefix, 64 columns per round);
//   phase 2  the DP table as a skewed pipeline over the lanes.  The reference's columns are dealt to the lanes in blocks of
//            C = 1, 2, 4, 8 or 16 consecutive columns (the smallest C with 64 C >= the width), each lane keeps its block of
//            the current DP row and its reference tokens in registers.  At step s lane l works on hypothesis row s - l: it
//            takes the hypothesis token and the cell left of its block from lane l - 1 (DPP wave_shr:1, no LDS), updates
//            its C cells and hands its last cell on.  n rows finish in n + (lanes in use) - 1 steps.  Lane 0's inputs (the
//            row's token, its boundary cell) are read from LDS 64 rows at a time and picked with v_readlane.
//            References wider than 1 024 columns (64 lanes x 16) are processed in strips of 1 024: the last lane of a strip
//            leaves its column in LDS as the next strip's boundary.
// Results leave with ordinary vector stores; the totals with 64-bit integer atomics (order-independent).
// The second kernel of the file aligns WORDS instead of tokens (WER) with the same two helpers; its phases and
// its LDS figure (3 KiB for a WSJ-like pair, 80 KiB at the limit) stand in front of it.
#include "common.h"

namespace {

constexpr int ED_MAX = ASR_ED_MAX_COLS;    // raw columns per row = entries of each LDS array
constexpr int ED_CMAX = 16;                // columns per lane at most
constexpr int ED_STRIP = 64 * ED_CMAX;     // reference columns per strip

struct EdArgs {
  int n_pairs;
  const void* hyp; int hyp_wide; int64_t ldh; int hyp_cols;
  const int32_t* hyp_len;
  const int32_t* ref; int64_t ldr; const int32_t* ref_len;
  const int32_t* ref_of_pair;
  int eos;
  const uint8_t* skip; int V;
  int32_t* dist; int32_t* hyp_n; int32_t* ref_n;
  unsigned long long* totals;
};

// lane l takes lane l-1's v; lane 0 (no source lane: the DPP leaves `old` in place) takes first
__device__ __forceinline__ int ed_shr1(int v, int first) {
  return __builtin_amdgcn_update_dpp(first, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

// Tokens of one row -> dst[0 .. count): columns [0, limit), cut before the first `eos` (eos < 0: no cut), tokens of the skip
// table dropped.  `load(c)` reads column c.  Returns the count (wave-uniform).
template <typename Load>
__device__ __forceinline__ int ed_compact(Load load, int limit, int eos, const uint8_t* __restrict__ skip, int V, int* dst,
                                          int lane) {
  int count = 0;
  for (int base = 0; base < limit; base += 64) {
    const int c = base + lane;
    const bool valid = c < limit;
    const int t = valid ? load(c) : 0;
    const unsigned long long ends = __ballot(valid && eos >= 0 && t == eos);
    const int first_end = ends ? __builtin_ctzll(ends) : 64;
    bool keep = valid && lane < first_end;
    if (keep && skip && t >= 0 && t < V) keep = skip[t] == 0;
    const unsigned long long kept = __ballot(keep);
    if (keep) dst[count + __popcll(kept & ((1ull << lane) - 1ull))] = t;
    count += __popcll(kept);
    if (ends) break;                                     // wave-uniform
  }
  return count;
}

// One strip of the table: reference columns col0 .. col0 + W - 1 (1-based DP columns col0 + 1 .. col0 + W), all n rows.
// bnd[i] holds D[i + 1][col0] on entry; with write_bnd the strip is full (W = ED_STRIP, C = ED_CMAX) and lane 63 leaves
// D[i + 1][col0 + W] there.  Returns D[n][col0 + W] in every lane.
template <int C>
__device__ __forceinline__ int ed_strip(const int* hyp_s, const int* ref_s, int* bnd, int n, int m, int col0, bool write_bnd,
                                        int lane) {
  const int W = min(m - col0, ED_STRIP);
  int r[C], row[C];
#pragma unroll
  for (int j = 0; j < C; ++j) {
    const int c = col0 + lane * C + j;
    r[j] = c < m ? ref_s[c] : 0;
    row[j] = c + 1;                                      // D[0][c + 1]
  }
  int diag = col0 + lane * C;                            // D[row done last][the column left of the block]
  const int lanes = (W + C - 1) / C;
  const int steps = n + lanes - 1;
  int x = 0, out = 0;
  for (int s0 = 0; s0 < steps; s0 += 64) {
    const int i0 = s0 + lane;
    const int hreg = i0 < n ? hyp_s[i0] : 0;
    const int breg = i0 < n ? bnd[i0] : 0;
    const int kend = min(64, steps - s0);
    for (int k = 0; k < kend; ++k) {
      x = ed_shr1(x, __builtin_amdgcn_readlane(hreg, k));
      const int left = ed_shr1(out, __builtin_amdgcn_readlane(breg, k));
      const int i = s0 + k - lane;
      if ((unsigned)i < (unsigned)n) {
        int d = diag, lf = left;
#pragma unroll
        for (int j = 0; j < C; ++j) {
          const int up = row[j];
          const int v = min(min(up, lf) + 1, d + (x != r[j] ? 1 : 0));
          d = up;
          lf = v;
          row[j] = v;
        }
        diag = left;
        out = lf;
        if (write_bnd && lane == 63) bnd[i] = lf;
      }
    }
  }
  const int q = W - 1;                                   // the strip's last column: lane q / C, register q % C
  int res = row[0];
#pragma unroll
  for (int j = 1; j < C; ++j) res = (q % C) == j ? row[j] : res;
  return __shfl(res, q / C, 64);
}

__global__ __launch_bounds__(64) void edit_distance_kernel(EdArgs a) {
  __shared__ int hyp_s[ED_MAX], ref_s[ED_MAX], bnd[ED_MAX];
  const int p = blockIdx.x, lane = threadIdx.x;
  const int64_t rrow = a.ref_of_pair ? a.ref_of_pair[p] : p;

  int hlim = a.hyp_len ? a.hyp_len[p] : a.hyp_cols;
  hlim = max(0, min(hlim, a.hyp_cols));
  int n;
  if (a.hyp_wide) {
    const int64_t* h = (const int64_t*)a.hyp + (int64_t)p * a.ldh;
    n = ed_compact([=](int c) { return (int)h[c]; }, hlim, a.eos, a.skip, a.V, hyp_s, lane);
  } else {
    const int32_t* h = (const int32_t*)a.hyp + (int64_t)p * a.ldh;
    n = ed_compact([=](int c) { return (int)h[c]; }, hlim, a.eos, a.skip, a.V, hyp_s, lane);
  }
  const int rlim = (int)max((int64_t)0, min((int64_t)a.ref_len[rrow], min(a.ldr, (int64_t)ED_MAX)));
  const int32_t* rf = a.ref + rrow * a.ldr;
  const int m = ed_compact([=](int c) { return (int)rf[c]; }, rlim, -1, a.skip, a.V, ref_s, lane);
  for (int i = lane; i < n; i += 64) bnd[i] = i + 1;     // D[i + 1][0]
  __syncthreads();

  int d = n;                                             // m == 0
  if (n == 0) d = m;
  else
    for (int col0 = 0; col0 < m; col0 += ED_STRIP) {
      const int W = min(m - col0, ED_STRIP);
      const bool more = col0 + ED_STRIP < m;
      if (W <= 64) d = ed_strip<1>(hyp_s, ref_s, bnd, n, m, col0, false, lane);
      else if (W <= 128) d = ed_strip<2>(hyp_s, ref_s, bnd, n, m, col0, false, lane);
      else if (W <= 256) d = ed_strip<4>(hyp_s, ref_s, bnd, n, m, col0, false, lane);
      else if (W <= 512) d = ed_strip<8>(hyp_s, ref_s, bnd, n, m, col0, false, lane);
      else d = ed_strip<ED_CMAX>(hyp_s, ref_s, bnd, n, m, col0, more, lane);
      if (more) __syncthreads();                         // lane 63's column is the next strip's boundary
    }

  if (lane == 0) {
    a.dist[p] = d;
    if (a.hyp_n) a.hyp_n[p] = n;
    if (a.ref_n) a.ref_n[p] = m;
    if (a.totals) {
      atomicAdd(a.totals, (unsigned long long)d);
      atomicAdd(a.totals + 1, (unsigned long long)m);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// The same distance on WORDS (the scoring half of WER): asr_word_edit_distance_i32.  One wave per pair again:
//   phase 1  both sides compacted as above into one LDS token row, the reference first;
//   phase 2  words: a token that is not `space` starts a word when it has no such token before it and ends one when it has
//            none behind it (ballot of the starts + popcount prefix = the word's index, 64 tokens per round; a word may
//            start in one round and end in a later one).  The words of both sides go into ONE list, the reference's first;
//   phase 3  a hash per word (one lane per word), then every word takes as its id the index of the first earlier word of
//            the reference with the same hash, length AND tokens - the hash only spares token compares, the tokens decide -
//            or its own index.  Only hypothesis-to-reference equality enters the table, so a hypothesis word is looked up
//            among the reference's words alone;
//   phase 4  the table on the ids, through ed_strip as above (at most 2 048 words a side: two strips).
// LDS is sized by the launch from the raw widths (cr = ldr, ch = hyp_cols columns; wr = (cr + 1) / 2, wh = (ch + 1) / 2
// words at most): tokens 4 (cr + ch) bytes, word start and end 2 x 2 (wr + wh), hash and id 2 x 4 (wr + wh); the boundary
// column (4 wh) lies over the starts and ends, which are dead by then.  A WSJ-like pair (150 columns a side) takes 3 KiB;
// the limit, 4 096 columns a side, 80 KiB = 32 + 16 + 32, half of a CU's 160 KiB.
struct WedArgs {
  EdArgs e;
  int space;
  int ref_cap, hyp_cap;                    // cr, ch: entries of the two token rows
};

// Words of the compacted row tok[0 .. ntok): word w's tokens are tok[wstart[w] - off .. wend[w] - off).  Returns the count.
__device__ __forceinline__ int ed_words(const int* tok, int ntok, int off, int space, unsigned short* wstart,
                                        unsigned short* wend, int lane) {
  const unsigned long long below = (1ull << lane) - 1ull;
  int count = 0;
  for (int base = 0; base < ntok; base += 64) {
    const int i = base + lane;
    const bool in_word = i < ntok && tok[i] != space;
    const bool start = in_word && (i == 0 || tok[i - 1] == space);
    const bool end = in_word && (i + 1 == ntok || tok[i + 1] == space);
    const unsigned long long starts = __ballot(start);
    const int before = count + __popcll(starts & below);               // words that start left of this token
    if (start) wstart[before] = (unsigned short)(off + i);
    if (end) wend[before + (start ? 1 : 0) - 1] = (unsigned short)(off + i + 1);
    count += __popcll(starts);
  }
  return count;
}

// The whole table over hyp_s[0 .. n) x ref_s[0 .. m), bnd[i] = i + 1 on entry: the strips of edit_distance_kernel.
__device__ __forceinline__ int ed_table(const int* hyp_s, const int* ref_s, int* bnd, int n, int m, int lane) {
  if (n == 0) return m;
  int d = n;                                                           // m == 0
  for (int col0 = 0; col0 < m; col0 += ED_STRIP) {
    const int W = min(m - col0, ED_STRIP);
    const bool more = col0 + ED_STRIP < m;
    if (W <= 64) d = ed_strip<1>(hyp_s, ref_s, bnd, n, m, col0, false, lane);
    else if (W <= 128) d = ed_strip<2>(hyp_s, ref_s, bnd, n, m, col0, false, lane);
    else if (W <= 256) d = ed_strip<4>(hyp_s, ref_s, bnd, n, m, col0, false, lane);
    else if (W <= 512) d = ed_strip<8>(hyp_s, ref_s, bnd, n, m, col0, false, lane);
    else d = ed_strip<ED_CMAX>(hyp_s, ref_s, bnd, n, m, col0, more, lane);
    if (more) __syncthreads();
  }
  return d;
}

__global__ __launch_bounds__(64) void word_edit_distance_kernel(WedArgs w) {
  extern __shared__ int wed_lds[];
  const EdArgs& a = w.e;
  const int nwords = (w.ref_cap + 1) / 2 + (w.hyp_cap + 1) / 2;
  int* tok = wed_lds;                                                  // [ref_cap | hyp_cap]
  unsigned* hash = (unsigned*)(tok + w.ref_cap + w.hyp_cap);           // [nwords]
  int* id = (int*)(hash + nwords);                                     // [nwords]
  unsigned short* wstart = (unsigned short*)(id + nwords);             // [nwords]
  unsigned short* wend = wstart + nwords;                              // [nwords]
  int* bnd = (int*)wstart;                                             // [(hyp_cap + 1) / 2], once the ids stand
  const int p = blockIdx.x, lane = threadIdx.x;
  const int64_t rrow = a.ref_of_pair ? a.ref_of_pair[p] : p;

  const int rlim = (int)max((int64_t)0, min((int64_t)a.ref_len[rrow], (int64_t)w.ref_cap));
  const int32_t* rf = a.ref + rrow * a.ldr;
  const int mt = ed_compact([=](int c) { return (int)rf[c]; }, rlim, -1, a.skip, a.V, tok, lane);
  int hlim = a.hyp_len ? a.hyp_len[p] : a.hyp_cols;
  hlim = max(0, min(hlim, a.hyp_cols));
  int nt;
  if (a.hyp_wide) {
    const int64_t* h = (const int64_t*)a.hyp + (int64_t)p * a.ldh;
    nt = ed_compact([=](int c) { return (int)h[c]; }, hlim, a.eos, a.skip, a.V, tok + w.ref_cap, lane);
  } else {
    const int32_t* h = (const int32_t*)a.hyp + (int64_t)p * a.ldh;
    nt = ed_compact([=](int c) { return (int)h[c]; }, hlim, a.eos, a.skip, a.V, tok + w.ref_cap, lane);
  }
  __syncthreads();

  const int m = ed_words(tok, mt, 0, w.space, wstart, wend, lane);
  const int n = ed_words(tok + w.ref_cap, nt, w.ref_cap, w.space, wstart + m, wend + m, lane);
  __syncthreads();

  for (int x = lane; x < m + n; x += 64) {
    const int s = wstart[x], len = wend[x] - s;
    unsigned h = (unsigned)len;
    for (int k = 0; k < len; ++k) h = asr_mix32(h + (unsigned)tok[s + k]);
    hash[x] = h;
  }
  __syncthreads();
  for (int x = lane; x < m + n; x += 64) {
    const int s = wstart[x], len = wend[x] - s;
    const unsigned h = hash[x];
    const int earlier = min(x, m);
    int first = x;
    for (int v = 0; v < earlier; ++v) {
      if (hash[v] != h) continue;
      const int sv = wstart[v];
      if (wend[v] - sv != len) continue;
      int k = 0;
      while (k < len && tok[sv + k] == tok[s + k]) ++k;
      if (k == len) {
        first = v;
        break;
      }
    }
    id[x] = first;
  }
  __syncthreads();                                                     // the starts and ends are dead: bnd takes their place
  for (int i = lane; i < n; i += 64) bnd[i] = i + 1;                   // D[i + 1][0]
  __syncthreads();

  const int d = ed_table(id + m, id, bnd, n, m, lane);
  if (lane == 0) {
    a.dist[p] = d;
    if (a.hyp_n) a.hyp_n[p] = n;
    if (a.ref_n) a.ref_n[p] = m;
    if (a.totals) {
      atomicAdd(a.totals, (unsigned long long)d);
      atomicAdd(a.totals + 1, (unsigned long long)m);
    }
  }
}

}  // namespace

extern "C" int asr_word_edit_distance_i32(int n_pairs, const void* hyp, int hyp_elem_bytes, int64_t ldh, int hyp_cols,
                                          const int32_t* hyp_len, const int32_t* ref, int64_t ldr, const int32_t* ref_len,
                                          const int32_t* ref_of_pair, int eos, const uint8_t* skip, int V, int space,
                                          int32_t* dist, int32_t* hyp_n, int32_t* ref_n, long long* totals,
                                          asr_stream_t stream_) {
  if (n_pairs <= 0 || !hyp || !ref || !ref_len || !dist || space < 0) return ASR_E_ARG;
  if ((hyp_elem_bytes != 4 && hyp_elem_bytes != 8) || hyp_cols < 0 || ldh < hyp_cols || ldr < 0) return ASR_E_ARG;
  if (hyp_cols > ED_MAX || ldr > ED_MAX) return ASR_E_SHAPE;
  WedArgs w;
  EdArgs& a = w.e;
  a.n_pairs = n_pairs;
  a.hyp = hyp; a.hyp_wide = hyp_elem_bytes == 8; a.ldh = ldh; a.hyp_cols = hyp_cols;
  a.hyp_len = hyp_len;
  a.ref = ref; a.ldr = ldr; a.ref_len = ref_len;
  a.ref_of_pair = ref_of_pair;
  a.eos = eos;
  a.skip = V > 0 ? skip : nullptr; a.V = V;
  a.dist = dist; a.hyp_n = hyp_n; a.ref_n = ref_n;
  a.totals = (unsigned long long*)totals;
  w.space = space;
  w.ref_cap = (int)ldr; w.hyp_cap = hyp_cols;
  const int nwords = (w.ref_cap + 1) / 2 + (w.hyp_cap + 1) / 2;
  const int lds = 4 * (w.ref_cap + w.hyp_cap) + 12 * nwords;
  if (lds > 64 * 1024) {                                               // beyond the default bound of dynamic LDS
    hipError_t e = hipFuncSetAttribute((const void*)word_edit_distance_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       4 * 2 * ED_MAX + 12 * ED_MAX);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(word_edit_distance_kernel, dim3(n_pairs), dim3(64), lds, (hipStream_t)stream_, w);
  ASR_CHECK_LAUNCH();
  return 0;
}

extern "C" int asr_edit_distance_i32(int n_pairs, const void* hyp, int hyp_elem_bytes, int64_t ldh, int hyp_cols,
                                     const int32_t* hyp_len, const int32_t* ref, int64_t ldr, const int32_t* ref_len,
                                     const int32_t* ref_of_pair, int eos, const uint8_t* skip, int V, int32_t* dist,
                                     int32_t* hyp_n, int32_t* ref_n, long long* totals, asr_stream_t stream_) {
  if (n_pairs <= 0 || !hyp || !ref || !ref_len || !dist) return ASR_E_ARG;
  if ((hyp_elem_bytes != 4 && hyp_elem_bytes != 8) || hyp_cols < 0 || ldh < hyp_cols || ldr < 0) return ASR_E_ARG;
  if (hyp_cols > ED_MAX || ldr > ED_MAX) return ASR_E_SHAPE;
  EdArgs a;
  a.n_pairs = n_pairs;
  a.hyp = hyp; a.hyp_wide = hyp_elem_bytes == 8; a.ldh = ldh; a.hyp_cols = hyp_cols;
  a.hyp_len = hyp_len;
  a.ref = ref; a.ldr = ldr; a.ref_len = ref_len;
  a.ref_of_pair = ref_of_pair;
  a.eos = eos;
  a.skip = V > 0 ? skip : nullptr; a.V = V;
  a.dist = dist; a.hyp_n = hyp_n; a.ref_n = ref_n;
  a.totals = (unsigned long long*)totals;
  hipLaunchKernelGGL(edit_distance_kernel, dim3(n_pairs), dim3(64), 0, (hipStream_t)stream_, a);
  ASR_CHECK_LAUNCH();
  return 0;
}
