// The per-layer launchers that more than one translation unit uses: the vocoder's per-op
// convolutions (vocoder.hip) and the strided Conv1d of the training losses with its backward
// (losses.hip).  Declarations only.
#pragma once

#include "losses_plan.h"

namespace m2 {

// vocoder.hip: Conv1d(k = 1 | 3, padding k / 2) + bias [* alpha + beta] [+ act] [+ residual], and
// ConvTranspose1d(k = 2 rate, stride rate, padding rate / 2) + bias [+ act]; PyTorch layouts.
int32_t launch_conv(const float* x, const float* w, const float* b, const float* alpha, const float* beta,
                    const float* res, int ksize, int act, bool x_transposed, int B, int Cin, int Cout, int L, float* y,
                    hipStream_t st);
int32_t launch_convT(const float* x, const float* w, const float* b, int rate, int act, int B, int Cin, int Cout, int L,
                     float* y, hipStream_t st);

namespace loss {

// One layer over nb utterances: y = leaky(conv(leaky(x, in_slope), w) + b, slope), x read through
// avg_pool1d(pool) (the direct kernel only); packed: w is [k, Cin/g, Cout] (MFMA path only); b may be null.
int32_t launch_conv(const float* x, const float* w, const float* b, float* y, const ConvGeo& g, int nb, int Lraw,
                    int pool, bool packed, float in_slope, float slope, hipStream_t st);

// The gradients of y = conv(leaky(x_pre, in_slope), w) + b over nb utterances: x_pre [nb, Cin, L],
// dy [nb, Cout, Lo]; dx (or null) is overwritten; dw (or null: no weight gradient, no partials) and db
// (or null) are overwritten or, with `accumulate`, added to.  part holds dw_plan's part_floats.
int32_t launch_conv_bwd(const float* x_pre, const float* w, const float* dy, const ConvGeo& g, int nb, int L,
                        bool packed, float in_slope, float* dx, float* dw, float* db, bool accumulate, float* part,
                        hipStream_t st);

// dw[i] = (accumulate ? dw[i] : 0) + part[0][i] + part[1][i] + ..., part [splits, n].
int32_t launch_dw_finish(const float* part, size_t n, int splits, bool accumulate, float* dw, hipStream_t st);

// db[co] = (accumulate ? db[co] : 0) + the sum of dy [nb, Cout, Lo] over utterances and positions.
int32_t launch_conv_db(const float* dy, int nb, int Cout, int Lo, bool accumulate, float* db, hipStream_t st);

}  // namespace loss
}  // namespace m2
