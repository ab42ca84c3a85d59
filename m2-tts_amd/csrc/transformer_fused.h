// Fused transformer-layer kernels (transformer_fused.hip).
#pragma once
#include <vector>

#include "m2_common.h"
#include "transformer_plan.h"

namespace m2 {

// The shape predicates (tf_fused_supported, tf_ln_gemm_supported,
// tf_post_next_supported, tf_src_fused_supported) are in transformer_plan.h.
// Every launcher's nw: waves per workgroup, 4 or 8 (the plan's row, tf_waves).

// W [N][K] row-major (nn.Linear.weight) -> B-fragment order for v_mfma_f32_16x16x4_f32.
std::vector<float> pack_bfrag(const float* W, int N, int K);
// W [N][K] -> the fused layers' split-f16 fragment order (same byte count as
// W in fp32); false if a weight is outside the f16 range.
bool pack_bfrag_split(const float* W, int N, int K, std::vector<float>* out);
// y[R][N] = LN(x)[R][K] . W^T (+ bias); Wp from pack_bfrag_split.
// (K, N) with an instance: (32, 96 | 32 | 64), (64, 192 | 64 | 80), (96, 288 | 80 | 96);
// any other answers M2_E_SHAPE (tf_ln_gemm_supported asks beforehand).
int32_t launch_ln_gemm(const float* x, const float* g, const float* b, const float* Wp, const float* bias, int act,
                       int R, int K, int N, int nw, float* y, hipStream_t st);
// y = o + FFN(LN2(o)), o = x + att . Wo^T + bo (Wo, W1, W2 from pack_bfrag_split); y may alias x.
int32_t launch_post_attn(const float* att, const float* x, const float* Wo, const float* bo, const float* g2,
                         const float* b2n, const float* W1, const float* b1, const float* W2, const float* b2, int R,
                         int H, int nw, float* y, hipStream_t st);
// post_attn followed, on the same row tile, by z = LN(y; gn, bn) . Wn^T (+ bn2)
// with NN output columns (the next layer's LN1 -> QKV, or the final LN -> mel).
int32_t launch_post_attn_next(const float* att, const float* x, const float* Wo, const float* bo, const float* g2,
                              const float* b2n, const float* W1, const float* b1, const float* W2, const float* b2,
                              int R, int H, int nw, float* y, const float* gn, const float* bn, const float* Wn,
                              const float* bn2, int NN, float* z, hipStream_t st);

// The first layer's LN1 -> QKV with its input rows built in the same launch
// (and stored to x, the residual input): the embedding + positional encoding +
// padding mask of the encoder (embed_pe_kernel), or the length regulator's
// frame expansion of the decoder (lr_expand_kernel).  (H, N) = (32, 96),
// (64, 192), (96, 288).
int32_t launch_embed_ln_gemm(const int64_t* ids, const float* emb, const float* pe, int B, int S, int H, int vocab,
                             const int64_t* lengths, uint8_t* mask, float* x, const float* g, const float* b,
                             const float* Wp, int N, int nw, float* y, hipStream_t st);
int32_t launch_expand_ln_gemm(const float* enc, const int32_t* cum, int B, int S, int T, int H, float* x,
                              const float* g, const float* b, const float* Wp, int N, int nw, float* y,
                              hipStream_t st);

}  // namespace m2
