// The device and launch side of layer_grad_plan.h, shared by decoder_grad.hip (which defines the
// launchers and their kernels) and encoder_grad.hip: the taped forward of one pre-LN layer, the walk
// of its backward steps, and the LayerNorm's backward over a workgroup's 64 whole rows, stated once
// for lin_dx_kernel's DX_LN epilogue and for ln_bwd_kernel.
#pragma once

#include "layer_grad_plan.h"

namespace m2 {
namespace dgrad {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The backward of LN(x) = x^ gamma + beta over the rows r0 .. r0 + 63 (those below R) of ln_x [R, K],
// K <= 16 KTM, 256 threads.  acc holds g_n, the cotangent of LN(x), as an MFMA accumulator: wave v the
// rows 16 v .., lane (g = lane / 16, li = lane % 16) the rows 4 g + r and the columns 16 t + li.  With
// a = g_n gamma, g_x = g_res + rstd (a - mean_k(a) - x^ mean_k(a x^)), g_res [R, K] or null; slots
// [2 K] (or null) receives the sum over the rows of g_n x^ (the first K) and of g_n.  g_x may be null
// (the slots alone).  sm: ln_lds_floats(K) floats, free for reuse once every thread has arrived.
template <int KTM>
__device__ __forceinline__ void ln_bwd_rows(const f32x4 (&acc)[KTM], float* sm, const float* __restrict__ ln_x,
                                            const float* __restrict__ gamma, const float* __restrict__ g_res, int R,
                                            int K, int r0, float* __restrict__ gx, float* __restrict__ slots) {
    const int kt = (K + 15) >> 4;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int lrow = wave * 16 + 4 * g;  // the lane's first row within the workgroup
    const int xs = K + 1;
    float* Xs = sm;                    // [64][K + 1]
    float* stats = Xs + kRows * xs;    // [64][2]: mean, rstd
    float* colp = stats + 2 * kRows;   // [4][2 K]: the waves' column sums
    __syncthreads();
    for (int i = tid; i < kRows * K; i += 256) {
        const int row = i / K, k = i - row * K;
        Xs[row * xs + k] = r0 + row < R ? ln_x[(size_t)(r0 + row) * K + k] : 0.f;
    }
    __syncthreads();
    {
        const int row = tid >> 2, part = tid & 3;
        const float* xr = Xs + row * xs;
        float s = 0.f;
        for (int k = part; k < K; k += 4) s += xr[k];
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        const float mean = s / (float)K;
        float v = 0.f;
        for (int k = part; k < K; k += 4) {
            const float dlt = xr[k] - mean;
            v = fmaf(dlt, dlt, v);
        }
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        if (part == 0) {
            stats[2 * row] = mean;
            stats[2 * row + 1] = 1.0f / sqrtf(v / (float)K + kLnEps);
        }
    }
    __syncthreads();
    float gam[KTM], cg[KTM], cb[KTM];
#pragma unroll
    for (int t = 0; t < KTM; ++t) {
        const int col = 16 * t + li;
        gam[t] = (t < kt && col < K) ? gamma[col] : 0.f;
        cg[t] = cb[t] = 0.f;
    }
    const float invK = 1.0f / (float)K;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = lrow + r;
        const float mean = stats[2 * row], rstd = stats[2 * row + 1];
        float xh[KTM], m1 = 0.f, m2 = 0.f;
#pragma unroll
        for (int t = 0; t < KTM; ++t) {
            const int col = 16 * t + li;
            xh[t] = (t < kt && col < K) ? (Xs[row * xs + col] - mean) * rstd : 0.f;
            const float a = acc[t][r] * gam[t];
            m1 += a;
            m2 = fmaf(a, xh[t], m2);
            cg[t] = fmaf(acc[t][r], xh[t], cg[t]);
            cb[t] += acc[t][r];
        }
        for (int o = 1; o < 16; o <<= 1) {
            m1 += __shfl_xor(m1, o);
            m2 += __shfl_xor(m2, o);
        }
        m1 *= invK;
        m2 *= invK;
        if (gx != nullptr && r0 + row < R) {
#pragma unroll
            for (int t = 0; t < KTM; ++t) {
                const int col = 16 * t + li;
                if (t < kt && col < K) {
                    const size_t o = (size_t)(r0 + row) * K + col;
                    const float v = rstd * (acc[t][r] * gam[t] - m1 - xh[t] * m2);
                    gx[o] = g_res ? g_res[o] + v : v;
                }
            }
        }
    }
    if (slots == nullptr) return;  // the same for every thread of the workgroup
#pragma unroll
    for (int t = 0; t < KTM; ++t) {
        cg[t] += __shfl_xor(cg[t], 16);
        cg[t] += __shfl_xor(cg[t], 32);
        cb[t] += __shfl_xor(cb[t], 16);
        cb[t] += __shfl_xor(cb[t], 32);
        const int col = 16 * t + li;
        if (g == 0 && t < kt && col < K) {
            colp[wave * 2 * K + col] = cg[t];
            colp[wave * 2 * K + K + col] = cb[t];
        }
    }
    __syncthreads();
    for (int i = tid; i < 2 * K; i += 256) slots[i] = ((colp[i] + colp[2 * K + i]) + colp[4 * K + i]) + colp[6 * K + i];
}

inline dim3 grid_of(const LaunchRow& r) { return dim3(r.gx, r.gy, r.gz); }

// dst = (add ? dst : 0) + the sum over `slots` partials of n floats, `stride` floats apart.
int32_t launch_finish(const float* part, size_t n, int slots, size_t stride, bool add, float* dst, hipStream_t st);
// The finishes of a LayerNorm's slots [blocks][2 K] into dgamma and dbeta (either may be null).
int32_t launch_ln_finish(const float* part, int K, int blocks, bool add, float* dgamma, float* dbeta, hipStream_t st);
// lin_dx_kernel and, in DX_LN mode, the finishes of its slots; part holds dx_part_floats.
int32_t launch_dx(const float* gy, const float* w, DxMode mode, const float* aux, const float* gamma, const float* g_res,
                  size_t R, int K, int N, float* gx, float* dgamma, float* dbeta, bool add, float* part, hipStream_t st);
// lin_dw_kernel and the finishes; part holds dw_split's part_floats.
int32_t launch_dw(const float* gy, const float* x, const float* ln_g, const float* ln_b, size_t R, int K, int N,
                  float* dw, float* db, bool add, float* part, hipStream_t st);
int32_t launch_att_bwd(const float* qkv, const uint8_t* mask, const float* att, const float* d_att, int B, int N, int H,
                       int heads, float* d_qkv, float* stats, hipStream_t st);

// One layer's forward on the per-op kernels, each op writing its map (m: the layer's five, MAP_*);
// p: the layer's 11 parameters; x its input; mask the key mask [B, N] or null.
int32_t layer_forward(const float* x, const float* const* p, float* const* m, const uint8_t* mask, int B, int N, int H,
                      int heads, hipStream_t st);

// What a walk over a plan's steps reads: the parameters and gradients by index, the tape's maps by
// index and the other buffers by -id (Buf).
struct Walk {
    const float* const* params;
    float* const* grads;  // a null entry: not wanted
    float* const* maps;
    float* named[kBufs];
    const uint8_t* mask;
    Geo geo;
    bool add;
    Bufs bufs;
    hipStream_t st;
    float* buf(int id) const { return id >= 0 ? maps[id] : named[-id]; }
    float* grad(int i) const { return i >= 0 ? grads[i] : nullptr; }
    const float* param(int i) const { return i >= 0 ? params[i] : nullptr; }
};
// Launches a STEP_DW, STEP_DX or STEP_ATT step; what was not asked for is skipped.
int32_t run_step(const Step& s, const Walk& w);

}  // namespace dgrad
}  // namespace m2
