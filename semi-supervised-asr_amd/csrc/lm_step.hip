// lm_step.hip — one step of one layer of the judge's stacked LSTM (LM.forward_step, model.py:534-542) for the R = B*K rows
// of a beam search with shallow fusion: gate products [x | h_prev] W_cat^T + b, the cell update and both
// writes of h_new in ONE launch; the gates never reach memory.
//   W_cat  [4H][In + H] = [W_ih | W_hh], rows gate-interleaved (row = unit * 4 + gate, gate in (i, f, g, o)), packed once
//          per search; b likewise, b_ih + b_hh.
// A workgroup owns 4 hidden units with all four gates (16 rows of W_cat: one 16-column MFMA tile, so the pointwise part
// needs no second pass) for MT * 16 rows, streams its 16 x (In + H) weight slice once and multiplies on the fp32-input
// MFMA (v_mfma_f32_16x16x4_f32: exact fp32 products) with K split over its waves - the skinny tile of common.h.
//   R <= 16   H / 4 workgroups of 8 waves: a weight-streaming problem (13 MB per layer at H = In = 640), each wave keeps
//             two groups of 8 float4 loads in flight per operand;
//   R <= 32   16-row workgroups of 4 waves, (H / 4) x 2;
//   R  > 32   32-row workgroups of 4 waves, (H / 4) x ceil(R / 32).
#include "common.h"

namespace {

template <int MT, int NW>
__global__ __launch_bounds__(NW * 64) void lm_step_kernel(int R, int H, int K, const float* __restrict__ xin, int64_t ldx,
                                                          const float* __restrict__ wcat, const float* __restrict__ bcat,
                                                          const float* __restrict__ cprev, float* __restrict__ cout,
                                                          float* __restrict__ hout, int64_t ldh,
                                                          float* __restrict__ hout2, int64_t ldh2) {
  __shared__ float red[NW * MT * 16 * SK_LDS_STRIDE];
  const int j = blockIdx.x;
  const int64_t row0 = (int64_t)blockIdx.y * (MT * 16);
  const int e = threadIdx.x;
  const int row = e >> 2, u = e & 3;
  const int64_t r = row0 + row;
  const int unit = 4 * j + u;
  const bool mine = e < MT * 64 && r < R;
  // epilogue operands first: their latency hides under the gate product
  float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
  float cp = 0.f;
  if (mine) {
    bb = *reinterpret_cast<const float4*>(bcat + unit * 4);
    cp = cprev[r * H + unit];
  }
  skinny_partial<MT, NW>(xin, ldx, row0, R, wcat, K, (int64_t)16 * j, (int64_t)4 * H, K, red);
  __syncthreads();
  if (mine) {
    const float gi = asr_sigmoid(skinny_reduced<MT, NW>(red, row, u * 4 + 0) + bb.x);
    const float gf = asr_sigmoid(skinny_reduced<MT, NW>(red, row, u * 4 + 1) + bb.y);
    const float gg = tanhf(skinny_reduced<MT, NW>(red, row, u * 4 + 2) + bb.z);
    const float go = asr_sigmoid(skinny_reduced<MT, NW>(red, row, u * 4 + 3) + bb.w);
    const float cn = gf * cp + gi * gg;
    const float hn = go * tanhf(cn);
    cout[r * H + unit] = cn;
    hout[r * ldh + unit] = hn;
    if (hout2) hout2[r * ldh2 + unit] = hn;   // the x part of the next layer's input row
  }
}

}  // namespace

extern "C" int asr_lm_step_f32(int R, int H, int In, const float* xin, int64_t ldx, const float* wcat, const float* bcat,
                               const float* c_prev, float* c_out, float* h_out, int64_t ldh, float* h_out2, int64_t ldh2,
                               asr_stream_t stream_) {
  if (!xin || !wcat || !bcat || !c_prev || !c_out || !h_out || R <= 0 || H <= 0 || In <= 0) return ASR_E_ARG;
  if (R > ASR_LM_MAX_ROWS || H % 16 || In % 16 || H > ASR_LM_MAX_WIDTH || In > ASR_LM_MAX_WIDTH) return ASR_E_SHAPE;
  if (ldx < In + H || ldh < H || (h_out2 && ldh2 < H)) return ASR_E_ARG;
  if (c_prev == c_out || xin == h_out || xin == h_out2) return ASR_E_ARG;          // a step reads one slot and writes another
  if (ldx % 4 || !asr_aligned16(xin) || !asr_aligned16(wcat) || !asr_aligned16(bcat)) return ASR_E_ALIGN;
  hipStream_t stream = (hipStream_t)stream_;
  const int K = In + H;
  const unsigned nj = (unsigned)(H / 4);
  if (R <= 16)
    hipLaunchKernelGGL((lm_step_kernel<1, 8>), dim3(nj, 1), dim3(512), 0, stream, R, H, K, xin, ldx, wcat, bcat, c_prev,
                       c_out, h_out, ldh, h_out2, ldh2);
  else if (R <= 32)
    hipLaunchKernelGGL((lm_step_kernel<1, 4>), dim3(nj, (unsigned)((R + 15) / 16)), dim3(256), 0, stream, R, H, K, xin, ldx,
                       wcat, bcat, c_prev, c_out, h_out, ldh, h_out2, ldh2);
  else
    hipLaunchKernelGGL((lm_step_kernel<2, 4>), dim3(nj, (unsigned)((R + 31) / 32)), dim3(256), 0, stream, R, H, K, xin, ldx,
                       wcat, bcat, c_prev, c_out, h_out, ldh, h_out2, ldh2);
  ASR_CHECK_LAUNCH();
  return 0;
}
