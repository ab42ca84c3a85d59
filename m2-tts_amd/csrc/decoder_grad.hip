// The training side of MelDecoder: a forward that keeps a tape, from the 11 layers + 4 raw
// parameters (no model handle: an optimizer step changes every one of them), and the gradient
// with respect to those parameters and the input x.  Exact f32 throughout, no floating-point
// atomics: every reduction over rows goes through partials in the workspace that are added in a
// fixed order, so equal inputs give equal bits, and a row of d_x depends on its own utterance only.
//
//   forward   the per-op path of a stand-alone MelDecoder (launch_linear with its fused LayerNorm,
//             ReLU and residual, launch_attention under the process's switches), each op writing
//             into the tape (decoder_grad_plan.h states the maps).
//   backward  plan_steps() in order.  Its kernels, all on v_mfma_f32_16x16x4_f32:
//             lin_dx_kernel      g_x [R, K] = g_y [R, N] W [N, K], W as stored, N chunked through
//                                LDS.  Epilogues: relu' from the taped h; or the backward of the
//                                LayerNorm the linear consumed, the workgroup holding whole rows:
//                                g_n never reaches HBM, and the workgroup's sums over its rows of
//                                g_n x^ and g_n go to one slot of the workspace.
//             lin_dw_kernel      partials of dW [N, K] = g_y^T X and db = sum_r g_y in one pass
//                                over g_y; X a taped map, or LN(x) re-formed while loading.
//             att_bwd_q_kernel   64 queries of one (utterance, head), keys streamed twice: the row
//                                max and sum, then P, dP = dO V^T, dS = P (dP - D), dQ = scale dS K.
//             att_bwd_kv_kernel  64 keys, queries streamed: P^T from the stored statistics,
//                                dV = P^T dO, dK = scale dS^T Q.
//             dec_finish_kernel  the sum of partials in a fixed order, stored or added.
// One MFMA accumulates a 16 x 16 tile D[i][j] += sum_k A[i][k] B[k][j], k < 4: lane (g = lane / 16,
// li = lane % 16) supplies A[li][g] and B[g][li] and holds D[4 g + r][li], r < 4.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "decoder_grad_plan.h"
#include "layer_grad.h"

namespace m2 {

int32_t launch_linear(const float*, const float*, const float*, const float*, const float*, const float*, int, int, int,
                      int, float*, hipStream_t);
int32_t launch_attention(const float*, const uint8_t*, int, int, int, int, float*, hipStream_t, bool force_f32 = false);

namespace dgrad {

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

constexpr float kLog2e = 1.4426950408889634f;  // softmax in base 2, as attention_kernel
constexpr int kTs = kRows + 4;                 // row stride of a transposed attention operand [hd][64]

// acc[t][r] += sum over the chunk's `red` reduction indices of As[k][i0 + 4 g + r] Bs[k][16 t + li]:
// As [red][kSa] (the caller passes As + i0), Bs [red][sb]; step s takes k = 4 s + g.
template <int KTM>
__device__ __forceinline__ void mma_chunk(f32x4 (&acc)[KTM], const float* As, const float* Bs, int sb, int kt, int red,
                                          int lane) {
    const int li = lane & 15, g = lane >> 4;
    for (int s = 0; s < red; s += 4) {
        const float a = As[(s + g) * kSa + li];
        const float* br = Bs + (s + g) * sb + li;
#pragma unroll
        for (int t = 0; t < KTM; ++t)
            if (t < kt) acc[t] = mfma16(a, br[16 * t], acc[t]);
    }
}

// grid (cdiv(R, 64)), 256 threads, dx_lds_bytes.  g_x [R, K] = g_y [R, N] w [N, K]; wave v takes the
// rows 16 v .. 16 v + 15 of the workgroup's 64 and every column.  K % 8 == 0, K <= 16 KTM.
//   relu_of [R, K]   g_x *= (relu_of > 0)
//   ln_x [R, K]      (K <= 128) the accumulator is g_n, the cotangent of LN(ln_x) = x^ gamma + beta:
//                    with a = g_n gamma, g_x = g_res + rstd (a - mean_k(a) - x^ mean_k(a x^)), g_res
//                    [R, K] or null; slots [gridDim.x][2 K] receives the workgroup's sum over its rows
//                    of g_n x^ (the first K) and of g_n.  g_x may be null (the slots alone).
template <int KTM>
__global__ __launch_bounds__(256) void lin_dx_kernel(const float* __restrict__ gy, const float* __restrict__ w,
                                                     const float* __restrict__ relu_of, const float* __restrict__ ln_x,
                                                     const float* __restrict__ gamma, const float* __restrict__ g_res,
                                                     int R, int K, int N, float* __restrict__ gx,
                                                     float* __restrict__ slots) {
    extern __shared__ float sm[];
    const int kt = (K + 15) >> 4, sb = 16 * kt + ((kt & 1) ? 0 : 16);
    float* As = sm;               // [kNc][kSa]: g_y transposed, As[n][row]
    float* Bs = sm + kNc * kSa;   // [kNc][sb]: w rows
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int r0 = blockIdx.x * kRows;
    f32x4 acc[KTM];
#pragma unroll
    for (int t = 0; t < KTM; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int n0 = 0; n0 < N; n0 += kNc) {
        __syncthreads();
        for (int i = tid; i < kRows * kNc; i += 256) {
            const int c = i & (kNc - 1), row = i / kNc, n = n0 + c;
            As[c * kSa + row] = (r0 + row < R && n < N) ? gy[(size_t)(r0 + row) * N + n] : 0.f;
        }
        const int wcols = 16 * kt;
        for (int i = tid; i < kNc * wcols; i += 256) {
            const int c = i / wcols, k = i - c * wcols, n = n0 + c;
            Bs[c * sb + k] = (n < N && k < K) ? w[(size_t)n * K + k] : 0.f;
        }
        __syncthreads();
        mma_chunk<KTM>(acc, As + wave * 16, Bs, sb, kt, kNc, lane);
    }
    const int lrow = wave * 16 + 4 * g;  // the lane's first row within the workgroup
    if (ln_x == nullptr) {
#pragma unroll
        for (int t = 0; t < KTM; ++t) {
            const int col = 16 * t + li;
            if (t < kt && col < K)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = r0 + lrow + r;
                    if (row < R) {
                        const size_t o = (size_t)row * K + col;
                        float v = acc[t][r];
                        if (relu_of) v = relu_of[o] > 0.f ? v : 0.f;
                        gx[o] = v;
                    }
                }
        }
        return;
    }
    // the LayerNorm's backward over the workgroup's whole rows
    ln_bwd_rows<KTM>(acc, sm, ln_x, gamma, g_res, R, K, r0, gx,
                     slots ? slots + (size_t)blockIdx.x * 2 * K : nullptr);
}

// grid (cdiv(N, 64), splits), 256 threads, DwPlan's lds.  Workgroup (bx, by) takes the rows
// [by rps, min(R, (by + 1) rps)) and the outputs n0 = 64 bx .. n0 + 63, wave v the 16 of them from
// 16 v, every column: partW [splits][N][K] += g_y[r][n] X[r][k], partB [splits][N] += g_y[r][n]
// (either may be null).  X = x [R, K], or with ln_g LN(x; ln_g, ln_b) re-formed row by row as the
// chunk is staged (K <= 256 either way).
template <int KTM>
__global__ __launch_bounds__(256) void lin_dw_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                     const float* __restrict__ ln_g, const float* __restrict__ ln_b,
                                                     int R, int K, int N, int rps, float* __restrict__ partW,
                                                     float* __restrict__ partB) {
    extern __shared__ float sm[];
    const int kt = (K + 15) >> 4, sb = 16 * kt + ((kt & 1) ? 0 : 16);
    float* As = sm;               // [kRc][kSa]: As[r][n]
    float* Bs = sm + kRc * kSa;   // [kRc][sb]: X rows
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * kRows;
    const int rbeg = blockIdx.y * rps, rend = min(R, rbeg + rps);
    f32x4 acc[KTM];
#pragma unroll
    for (int t = 0; t < KTM; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    const int wcols = 16 * kt;
    for (int rc = rbeg; rc < rend; rc += kRc) {
        __syncthreads();
        for (int i = tid; i < kRc * kRows; i += 256) {
            const int rr = i / kRows, c = i & (kRows - 1), n = n0 + c;
            As[rr * kSa + c] = (rc + rr < rend && n < N) ? gy[(size_t)(rc + rr) * N + n] : 0.f;
        }
        for (int i = tid; i < kRc * wcols; i += 256) {
            const int rr = i / wcols, k = i - rr * wcols;
            Bs[rr * sb + k] = (rc + rr < rend && k < K) ? x[(size_t)(rc + rr) * K + k] : 0.f;
        }
        __syncthreads();
        if (ln_g != nullptr) {  // eight lanes per row
            const int rr = tid >> 3, part = tid & 7;
            float* xr = Bs + rr * sb;
            float s = 0.f;
            for (int k = part; k < K; k += 8) s += xr[k];
            for (int o = 1; o < 8; o <<= 1) s += __shfl_xor(s, o);
            const float mean = s / (float)K;
            float v = 0.f;
            for (int k = part; k < K; k += 8) {
                const float dlt = xr[k] - mean;
                v = fmaf(dlt, dlt, v);
            }
            for (int o = 1; o < 8; o <<= 1) v += __shfl_xor(v, o);
            const float rstd = 1.0f / sqrtf(v / (float)K + kLnEps);
            for (int k = part; k < K; k += 8) xr[k] = (xr[k] - mean) * rstd * ln_g[k] + ln_b[k];
            __syncthreads();
        }
        mma_chunk<KTM>(acc, As + wave * 16, Bs, sb, kt, kRc, lane);
        if (tid < kRows)
            for (int rr = 0; rr < kRc; ++rr) bsum += As[rr * kSa + tid];
    }
    if (partW != nullptr) {
        float* pw = partW + (size_t)blockIdx.y * N * K;
#pragma unroll
        for (int t = 0; t < KTM; ++t) {
            const int col = 16 * t + li;
            if (t < kt && col < K)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = n0 + wave * 16 + 4 * g + r;
                    if (n < N) pw[(size_t)n * K + col] = acc[t][r];
                }
        }
    }
    if (partB != nullptr && tid < kRows && n0 + tid < N) partB[(size_t)blockIdx.y * N + n0 + tid] = bsum;
}

// grid (cdiv(n, kFinE)), 256 threads: kFinE elements by kFinG groups of slots.  Group q adds the slots
// q, q + kFinG, ... of its element in that order, the groups' sums are added as a fixed tree, and
// dst[i] = (add ? dst[i] : 0) + that sum, i < n; slot k of element i is part[k stride + i].
__global__ __launch_bounds__(256) void dec_finish_kernel(const float* __restrict__ part, size_t n, int slots,
                                                         size_t stride, int add, float* __restrict__ dst) {
    __shared__ float red[kFinG][kFinE];
    const int e = threadIdx.x % kFinE, q = threadIdx.x / kFinE;
    const size_t i = (size_t)blockIdx.x * kFinE + e;
    float s = 0.f;
    if (i < n)
        for (int k = q; k < slots; k += kFinG) s += part[(size_t)k * stride + i];
    red[q][e] = s;
    __syncthreads();
    for (int h = kFinG / 2; h > 0; h >>= 1) {
        if (q < h) red[q][e] += red[q + h][e];
        __syncthreads();
    }
    if (q == 0 && i < n) dst[i] = add ? dst[i] + red[0][e] : red[0][e];
}

// A chunk of 64 rows (j0 ..) of one third of qkv, or of a [B, N, H] map, of one (utterance, head),
// transposed into dst [HD][kTs]; rows past N are 0.  src points at row 0's first head column.
template <int HD>
__device__ __forceinline__ void stash_t(float* dst, const float* src, size_t row_stride, int j0, int N, int tid) {
    for (int i = tid; i < kRows * (HD / 4); i += 256) {
        const int row = i / (HD / 4), d4 = i - row * (HD / 4), j = j0 + row;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < N) v = *reinterpret_cast<const float4*>(src + (size_t)j * row_stride + 4 * d4);
        dst[(4 * d4 + 0) * kTs + row] = v.x;
        dst[(4 * d4 + 1) * kTs + row] = v.y;
        dst[(4 * d4 + 2) * kTs + row] = v.z;
        dst[(4 * d4 + 3) * kTs + row] = v.w;
    }
}

// One 16 x 16 tile of X Y^T over the head dimension: rows are 16 LDS rows of Xt [HD][kTs] (column
// c0 + li), columns the lanes' own rows y[t] (y[t] = Y[li][16 t + 4 g ..]): out[r] = (4 g + r, li).
template <int HD>
__device__ __forceinline__ f32x4 dot_tile(const float* Xt, int c0, const float4 (&y)[HD / 16], int li, int g) {
    f32x4 st = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < HD / 16; ++t) {
        const float* a = Xt + (16 * t + 4 * g) * kTs + c0 + li;
        st = mfma16(a[0], y[t].x, st);
        st = mfma16(a[kTs], y[t].y, st);
        st = mfma16(a[2 * kTs], y[t].z, st);
        st = mfma16(a[3 * kTs], y[t].w, st);
    }
    return st;
}

// acc[t] (rows d = 16 t + 4 g + r, column li) += sum over the 16 LDS columns c0 .. of Xt[d][c0 + 4 g + r]
// times the lane's p[r]: the product X^T P with P straight from a dot_tile's accumulator.
template <int HD>
__device__ __forceinline__ void acc_tile(f32x4 (&acc)[HD / 16], const float* Xt, int c0, const float (&p)[4], int li,
                                         int g) {
#pragma unroll
    for (int t = 0; t < HD / 16; ++t) {
        const float4 v = *reinterpret_cast<const float4*>(Xt + (16 * t + li) * kTs + c0 + 4 * g);
        acc[t] = mfma16(v.x, p[0], acc[t]);
        acc[t] = mfma16(v.y, p[1], acc[t]);
        acc[t] = mfma16(v.z, p[2], acc[t]);
        acc[t] = mfma16(v.w, p[3], acc[t]);
    }
}

// grid (cdiv(N, 64), heads, B), 256 threads, att_lds_bytes.  qkv [B, N, 3 H], att and d_att [B, N, H],
// key_mask [B, N] (0: masked) or null.  Wave v takes the queries 16 v .. of the workgroup's 64; a lane
// holds query li's scores of the keys 4 g + r of each 16-key block, as attention_kernel.  Scores are
// (q.k) scale log2(e), masked keys exactly -1e9 log2(e).  dS of a masked key is 0 by definition (the
// forward replaces its score).  Writes the q third of d_qkv and stats [B, heads, N, 3] = row max,
// 1 / row sum, D = sum_d dO o.
template <int HD>
__global__ __launch_bounds__(256) void att_bwd_q_kernel(const float* __restrict__ qkv,
                                                        const uint8_t* __restrict__ key_mask,
                                                        const float* __restrict__ att, const float* __restrict__ d_att,
                                                        int N, int H, float scale, float* __restrict__ d_qkv,
                                                        float* __restrict__ stats) {
    constexpr int NT = HD / 16;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Kt = sm;                 // [HD][kTs]
    float* Vt = sm + HD * kTs;      // [HD][kTs]
    float* Mk = Vt + HD * kTs;      // [64]: 0 live, 1 masked, 2 past the end
    const int b = blockIdx.z, hh = blockIdx.y, heads = gridDim.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    const size_t row3 = (size_t)3 * H;
    const float* base = qkv + (size_t)b * N * row3 + hh * HD;
    const int qi = blockIdx.x * kRows + wave * 16 + li;
    const float sl2 = scale * kLog2e;
    float4 q[NT], dO[NT];
    float D = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        q[t] = dO[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (qi < N) {
            const size_t o = ((size_t)b * N + qi) * H + hh * HD + 16 * t + 4 * g;
            q[t] = *reinterpret_cast<const float4*>(base + (size_t)qi * row3 + 16 * t + 4 * g);
            dO[t] = *reinterpret_cast<const float4*>(d_att + o);
            const float4 ov = *reinterpret_cast<const float4*>(att + o);
            D = fmaf(dO[t].x, ov.x, fmaf(dO[t].y, ov.y, fmaf(dO[t].z, ov.z, fmaf(dO[t].w, ov.w, D))));
        }
    }
    D += __shfl_xor(D, 16);
    D += __shfl_xor(D, 32);
    auto stage = [&](int j0, bool with_v) {
        __syncthreads();
        stash_t<HD>(Kt, base + H, row3, j0, N, tid);
        if (with_v) stash_t<HD>(Vt, base + 2 * H, row3, j0, N, tid);
        if (tid < kRows) {
            const int j = j0 + tid;
            Mk[tid] = j >= N ? 2.f : ((key_mask && key_mask[(size_t)b * N + j] == 0) ? 1.f : 0.f);
        }
        __syncthreads();
    };
    auto scores = [&](int kb, float (&s)[4]) {
        const f32x4 st = dot_tile<HD>(Kt, 16 * kb, q, li, g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float mk = Mk[16 * kb + 4 * g + r];
            s[r] = mk == 0.f ? st[r] * sl2 : (mk == 1.f ? kMaskFill * kLog2e : -INFINITY);
        }
    };
    // pass 1: the row max and sum
    float m = -INFINITY, lsum = 0.f;
    for (int j0 = 0; j0 < N; j0 += kRows) {
        stage(j0, false);
        float s[4][4], cmax = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            scores(kb, s[kb]);
#pragma unroll
            for (int r = 0; r < 4; ++r) cmax = fmaxf(cmax, s[kb][r]);
        }
        cmax = fmaxf(cmax, __shfl_xor(cmax, 16));
        cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
        const float mn = fmaxf(m, cmax);
        lsum *= exp2f(m - mn);
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) lsum += exp2f(s[kb][r] - mn);
        m = mn;
    }
    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);
    const float inv = 1.0f / lsum;
    // pass 2: dS and dQ^T[d][q] = sum_key K^T[d][key] dS^T[key][q]
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < N; j0 += kRows) {
        stage(j0, true);
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            float s[4], ds[4];
            scores(kb, s);
            const f32x4 dp = dot_tile<HD>(Vt, 16 * kb, dO, li, g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = exp2f(s[r] - m) * inv;
                ds[r] = Mk[16 * kb + 4 * g + r] == 0.f ? p * (dp[r] - D) : 0.f;
            }
            acc_tile<HD>(acc, Kt, 16 * kb, ds, li, g);
        }
    }
    if (qi >= N) return;
    float* o = d_qkv + ((size_t)b * N + qi) * row3 + hh * HD;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[16 * t + 4 * g + r] = acc[t][r] * scale;
    if (g == 0) {
        float* sp = stats + (((size_t)b * heads + hh) * N + qi) * 3;
        sp[0] = m;
        sp[1] = inv;
        sp[2] = D;
    }
}

// grid (cdiv(N, 64), heads, B), 256 threads, att_lds_bytes.  Wave v takes the keys 16 v .. of the
// workgroup's 64, a lane key li's k and v rows in registers; queries stream through LDS in chunks
// of 64 with their statistics.  A lane holds P[q][key li] for the queries 4 g + r of each 16-query
// block, re-formed as exp2(s - max) / sum; dV^T[d][key] += dO^T[d][q] P[q][key] and
// dK^T[d][key] += Q^T[d][q] dS[q][key] take it straight from the accumulator.  Writes the k and v
// thirds of d_qkv.
template <int HD>
__global__ __launch_bounds__(256) void att_bwd_kv_kernel(const float* __restrict__ qkv,
                                                         const uint8_t* __restrict__ key_mask,
                                                         const float* __restrict__ d_att,
                                                         const float* __restrict__ stats, int N, int H, float scale,
                                                         float* __restrict__ d_qkv) {
    constexpr int NT = HD / 16;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Qt = sm;                 // [HD][kTs]
    float* dOt = sm + HD * kTs;     // [HD][kTs]
    float* St = dOt + HD * kTs;     // [3][64]: max, 1 / sum, D of the chunk's queries
    const int b = blockIdx.z, hh = blockIdx.y, heads = gridDim.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    const size_t row3 = (size_t)3 * H;
    const float* base = qkv + (size_t)b * N * row3 + hh * HD;
    const float* dob = d_att + (size_t)b * N * H + hh * HD;
    const float* sb = stats + ((size_t)b * heads + hh) * N * 3;
    const int key = blockIdx.x * kRows + wave * 16 + li;
    const float sl2 = scale * kLog2e;
    float4 kr[NT], vr[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        kr[t] = vr[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (key < N) {
            kr[t] = *reinterpret_cast<const float4*>(base + (size_t)key * row3 + H + 16 * t + 4 * g);
            vr[t] = *reinterpret_cast<const float4*>(base + (size_t)key * row3 + 2 * H + 16 * t + 4 * g);
        }
    }
    // 0 live, 1 masked, 2 past the end
    const int mk = key >= N ? 2 : ((key_mask && key_mask[(size_t)b * N + key] == 0) ? 1 : 0);
    f32x4 accK[NT], accV[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) accK[t] = accV[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int q0 = 0; q0 < N; q0 += kRows) {
        __syncthreads();
        stash_t<HD>(Qt, base, row3, q0, N, tid);
        stash_t<HD>(dOt, dob, (size_t)H, q0, N, tid);
        if (tid < kRows) {
            const int qq = q0 + tid;
            // a query past the end: 1 / sum = 0 makes its P and dS exactly 0
            St[tid] = qq < N ? sb[(size_t)qq * 3] : 0.f;
            St[kRows + tid] = qq < N ? sb[(size_t)qq * 3 + 1] : 0.f;
            St[2 * kRows + tid] = qq < N ? sb[(size_t)qq * 3 + 2] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) {
            const f32x4 st = dot_tile<HD>(Qt, 16 * qb, kr, li, g);
            const f32x4 dp = dot_tile<HD>(dOt, 16 * qb, vr, li, g);
            float p[4], ds[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qq = 16 * qb + 4 * g + r;
                const float s = mk == 0 ? st[r] * sl2 : kMaskFill * kLog2e;
                p[r] = mk == 2 ? 0.f : exp2f(s - St[qq]) * St[kRows + qq];
                ds[r] = mk == 0 ? p[r] * (dp[r] - St[2 * kRows + qq]) : 0.f;
            }
            acc_tile<HD>(accV, dOt, 16 * qb, p, li, g);
            acc_tile<HD>(accK, Qt, 16 * qb, ds, li, g);
        }
    }
    if (key >= N) return;
    float* o = d_qkv + ((size_t)b * N + key) * row3 + H + hh * HD;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            o[16 * t + 4 * g + r] = accK[t][r] * scale;
            o[H + 16 * t + 4 * g + r] = accV[t][r];
        }
}

// ---- the launchers (layer_grad.h) -----------------------------------------------------

int32_t launch_finish(const float* part, size_t n, int slots, size_t stride, bool add, float* dst, hipStream_t st) {
    const LaunchRow r = finish_row(n);
    hipLaunchKernelGGL(dec_finish_kernel, grid_of(r), dim3(r.threads), 0, st, part, n, slots, stride, add ? 1 : 0, dst);
    M2_LAUNCHED(r.kernel);
    return M2_OK;
}

int32_t launch_ln_finish(const float* part, int K, int blocks, bool add, float* dgamma, float* dbeta, hipStream_t st) {
    if (dgamma) {
        const int32_t rc = launch_finish(part, (size_t)K, blocks, (size_t)2 * K, add, dgamma, st);
        if (rc != M2_OK) return rc;
    }
    if (dbeta) return launch_finish(part + K, (size_t)K, blocks, (size_t)2 * K, add, dbeta, st);
    return M2_OK;
}

int32_t launch_dx(const float* gy, const float* w, DxMode mode, const float* aux, const float* gamma, const float* g_res,
                  size_t R, int K, int N, float* gx, float* dgamma, float* dbeta, bool add, float* part,
                  hipStream_t st) {
    const LaunchRow r = dx_row(R, K, mode);
    const float* relu_of = mode == DX_RELU ? aux : nullptr;
    const float* ln_x = mode == DX_LN ? aux : nullptr;
    float* slots = (dgamma || dbeta) ? part : nullptr;
    const int kt = col_tiles(K);
#define M2_DX(KTM)                                                                                             \
    hipLaunchKernelGGL(lin_dx_kernel<KTM>, grid_of(r), dim3(r.threads), r.lds, st, gy, w, relu_of, ln_x, gamma, \
                       g_res, (int)R, K, N, gx, slots)
    if (kt <= 4) M2_DX(4);
    else if (kt <= 8) M2_DX(8);
    else M2_DX(16);
#undef M2_DX
    M2_LAUNCHED(r.kernel);
    return launch_ln_finish(part, K, dx_blocks(R), add, dgamma, dbeta, st);
}

int32_t launch_dw(const float* gy, const float* x, const float* ln_g, const float* ln_b, size_t R, int K, int N,
                  float* dw, float* db, bool add, float* part, hipStream_t st) {
    const DwPlan p = dw_split(R, K, N);
    const size_t n = (size_t)N * K;
    float* partW = dw ? part : nullptr;
    float* partB = db ? part + (size_t)p.splits * n : nullptr;
    const dim3 grid(p.tiles, p.splits);
    const int kt = col_tiles(K);
#define M2_DW(KTM)                                                                                              \
    hipLaunchKernelGGL(lin_dw_kernel<KTM>, grid, dim3(256), p.lds, st, gy, x, ln_g, ln_b, (int)R, K, N, p.rps, \
                       partW, partB)
    if (kt <= 4) M2_DW(4);
    else if (kt <= 8) M2_DW(8);
    else M2_DW(16);
#undef M2_DW
    M2_LAUNCHED("lin_dw_kernel");
    if (dw) {
        const int32_t rc = launch_finish(partW, n, p.splits, n, add, dw, st);
        if (rc != M2_OK) return rc;
    }
    if (db) return launch_finish(partB, (size_t)N, p.splits, (size_t)N, add, db, st);
    return M2_OK;
}

template <int HD>
static int32_t launch_att_bwd_hd(const float* qkv, const uint8_t* mask, const float* att, const float* d_att, int B,
                                 int N, int H, int heads, float scale, float* d_qkv, float* stats, hipStream_t st) {
    const dim3 grid(cdiv(N, kRows), heads, B);
    const size_t lds = att_lds_bytes(HD);
    hipLaunchKernelGGL(att_bwd_q_kernel<HD>, grid, dim3(256), lds, st, qkv, mask, att, d_att, N, H, scale, d_qkv, stats);
    M2_LAUNCHED("att_bwd_q_kernel");
    hipLaunchKernelGGL(att_bwd_kv_kernel<HD>, grid, dim3(256), lds, st, qkv, mask, d_att, stats, N, H, scale, d_qkv);
    M2_LAUNCHED("att_bwd_kv_kernel");
    return M2_OK;
}

int32_t launch_att_bwd(const float* qkv, const uint8_t* mask, const float* att, const float* d_att, int B, int N, int H,
                       int heads, float* d_qkv, float* stats, hipStream_t st) {
    const int hd = H / heads;
    const float scale = (float)(1.0 / std::sqrt((double)hd));  // as launch_attention
    switch (hd) {
        case 16: return launch_att_bwd_hd<16>(qkv, mask, att, d_att, B, N, H, heads, scale, d_qkv, stats, st);
        case 32: return launch_att_bwd_hd<32>(qkv, mask, att, d_att, B, N, H, heads, scale, d_qkv, stats, st);
        case 48: return launch_att_bwd_hd<48>(qkv, mask, att, d_att, B, N, H, heads, scale, d_qkv, stats, st);
        case 64: return launch_att_bwd_hd<64>(qkv, mask, att, d_att, B, N, H, heads, scale, d_qkv, stats, st);
        default: return fail(M2_E_SHAPE, "attention backward: head_dim must be 16, 32, 48 or 64");
    }
}

int32_t layer_forward(const float* x, const float* const* p, float* const* m, const uint8_t* mask, int B, int N, int H,
                      int heads, hipStream_t st) {
    const int R = B * N;
    int32_t rc = launch_linear(x, p[P_N1_W], p[P_N1_B], p[P_QKV_W], nullptr, nullptr, ACT_NONE, R, H, 3 * H, m[MAP_QKV],
                               st);
    if (rc == M2_OK) rc = launch_attention(m[MAP_QKV], mask, B, N, H, heads, m[MAP_ATT], st);
    if (rc == M2_OK)
        rc = launch_linear(m[MAP_ATT], nullptr, nullptr, p[P_OUT_W], p[P_OUT_B], x, ACT_NONE, R, H, H, m[MAP_XMID], st);
    if (rc == M2_OK)
        rc = launch_linear(m[MAP_XMID], p[P_N2_W], p[P_N2_B], p[P_L1_W], p[P_L1_B], nullptr, ACT_RELU, R, H, 2 * H,
                           m[MAP_H], st);
    if (rc == M2_OK)
        rc = launch_linear(m[MAP_H], nullptr, nullptr, p[P_L2_W], p[P_L2_B], m[MAP_XMID], ACT_NONE, R, 2 * H, H,
                           m[MAP_XOUT], st);
    return rc;
}

int32_t run_step(const Step& s, const Walk& w) {
    const Geo& g = w.geo;
    switch (s.kind) {
        case STEP_DW:
            if (!w.grad(s.dw) && !w.grad(s.db)) return M2_OK;
            return launch_dw(w.buf(s.gy), w.buf(s.x), w.param(s.ln), s.ln >= 0 ? w.params[s.ln + 1] : nullptr, g.R, s.K,
                             s.N, w.grad(s.dw), w.grad(s.db), w.add, w.bufs.part, w.st);
        case STEP_DX: {
            float* out = w.buf(s.out);  // null only for layer 0's input when nothing asks for it
            if (!out && !w.grad(s.dgamma) && !w.grad(s.dbeta)) return M2_OK;
            return launch_dx(w.buf(s.gy), w.params[s.w], s.mode, w.buf(s.aux), w.param(s.dgamma), w.buf(s.res), g.R, s.K,
                             s.N, out, w.grad(s.dgamma), w.grad(s.dbeta), w.add, w.bufs.part, w.st);
        }
        case STEP_ATT:
            return launch_att_bwd(w.buf(s.x), w.mask, w.buf(s.aux), w.buf(s.gy), g.B, g.N, g.H, g.heads, w.bufs.wide,
                                  w.bufs.stats, w.st);
        default: return fail(M2_E_ARG, "run_step: not a step of the layer walk");
    }
}

}  // namespace dgrad
}  // namespace m2

namespace {
using namespace m2;
using dgrad::Dims;
using dgrad::DxMode;
using dgrad::launch_att_bwd;
using dgrad::launch_dw;
using dgrad::launch_dx;
using dgrad::Step;

const char* kDimsMsg = "H a multiple of 8 with 2 H <= 256, head_dim 16, 32, 48 or 64, M >= 1, layers >= 1";

size_t tape_bytes(const Dims& d) {
    Sizer s;
    dgrad::carve_tape(s, d, nullptr);
    return s.off + 256;
}

size_t backward_bytes(const Dims& d) {
    if (d.B == 0 || d.T == 0) return 256;
    Sizer s;
    dgrad::carve_backward(s, d, nullptr);
    return s.off + 256;
}
}  // namespace

extern "C" {

size_t m2_decoder_tape_bytes(int32_t H, int32_t M, int32_t layers, int32_t heads, int32_t B, int32_t T) {
    const Dims d{H, M, layers, heads, B, T};
    return dgrad::dims_ok(d) ? tape_bytes(d) : 0;
}

int32_t m2_decoder_tape_map(int32_t H, int32_t M, int32_t layers, int32_t heads, int32_t B, int32_t T, int32_t index,
                            size_t* offset_floats, int32_t* width) {
    const Dims d{H, M, layers, heads, B, T};
    M2_CHECK_SHAPE(dgrad::dims_ok(d), kDimsMsg);
    M2_CHECK_ARG(offset_floats && width && index >= 0 && index < dgrad::n_maps(d), "m2_decoder_tape_map: bad argument");
    Sizer s;  // carve_tape's arithmetic, map by map
    for (int i = 0; i <= index; ++i) {
        const size_t at = align_up(s.off, 256);
        s.take<float>(dgrad::rows(d) * dgrad::map_width(d, i));
        if (i == index) {
            *offset_floats = at / sizeof(float);
            *width = dgrad::map_width(d, i);
        }
    }
    return M2_OK;
}

int32_t m2_decoder_train_forward(const float* const* params, int32_t H, int32_t M, int32_t layers, int32_t heads,
                                 const float* x, int32_t B, int32_t T, float* mel, void* tape, size_t tape_bytes_,
                                 void* stream) {
    const Dims d{H, M, layers, heads, B, T};
    M2_CHECK_SHAPE(dgrad::dims_ok(d), kDimsMsg);
    if (B == 0 || T == 0) return M2_OK;
    M2_CHECK_ARG(params && x && mel && tape, "m2_decoder_train_forward: bad argument");
    for (int i = 0; i < dgrad::n_params(d); ++i) M2_CHECK_ARG(params[i], "m2_decoder_train_forward: null parameter");
    Carve c(tape, tape_bytes_);
    float* map[dgrad::kLayerMaps * dgrad::kMaxLayers];
    dgrad::carve_tape(c, d, map);
    if (!c.ok) return fail(M2_E_ARG, "m2_decoder_train_forward: tape too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int R = B * T;
    const float* cur = x;
    int32_t rc = M2_OK;
    for (int l = 0; l < layers && rc == M2_OK; ++l) {
        float** m = map + dgrad::map_of(l, 0);
        rc = dgrad::layer_forward(cur, params + dgrad::p_layer(l, 0), m, nullptr, B, T, H, heads, st);
        cur = m[dgrad::MAP_XOUT];
    }
    if (rc != M2_OK) return rc;
    const float* const* t = params + dgrad::p_tail(d, 0);
    return launch_linear(cur, t[dgrad::T_N_W], t[dgrad::T_N_B], t[dgrad::T_MEL_W], t[dgrad::T_MEL_B], nullptr, ACT_NONE,
                         R, H, M, mel, st);
}

size_t m2_decoder_backward_workspace_bytes(int32_t H, int32_t M, int32_t layers, int32_t heads, int32_t B, int32_t T) {
    const Dims d{H, M, layers, heads, B, T};
    return dgrad::dims_ok(d) ? backward_bytes(d) : 0;
}

int32_t m2_decoder_backward(const float* const* params, int32_t H, int32_t M, int32_t layers, int32_t heads,
                            const float* x, int32_t B, int32_t T, const void* tape, const float* d_mel, float* d_x,
                            float* const* grads, int32_t accumulate, void* workspace, size_t workspace_bytes,
                            void* stream) {
    const Dims d{H, M, layers, heads, B, T};
    M2_CHECK_SHAPE(dgrad::dims_ok(d), kDimsMsg);
    if (B == 0 || T == 0) return M2_OK;
    M2_CHECK_ARG(params && x && tape && d_mel && grads && workspace, "m2_decoder_backward: bad argument");
    for (int i = 0; i < dgrad::n_params(d); ++i) M2_CHECK_ARG(params[i], "m2_decoder_backward: null parameter");
    Sizer ts;
    dgrad::carve_tape(ts, d, nullptr);
    Carve tc(const_cast<void*>(tape), ts.off);
    float* map[dgrad::kLayerMaps * dgrad::kMaxLayers];
    dgrad::carve_tape(tc, d, map);
    Carve c(workspace, workspace_bytes);
    dgrad::Bufs bufs;
    dgrad::carve_backward(c, d, &bufs);
    if (!c.ok) return fail(M2_E_ARG, "m2_decoder_backward: workspace too small");
    dgrad::Walk w{};
    w.params = params;
    w.grads = grads;
    w.maps = map;
    w.named[-dgrad::BUF_X] = const_cast<float*>(x);
    w.named[-dgrad::BUF_DMEL] = const_cast<float*>(d_mel);
    w.named[-dgrad::BUF_DX] = d_x;
    w.named[-dgrad::BUF_COT0] = bufs.cot[0];
    w.named[-dgrad::BUF_COT1] = bufs.cot[1];
    w.named[-dgrad::BUF_WIDE] = bufs.wide;
    w.geo = dgrad::geo(d);
    w.add = accumulate != 0;
    w.bufs = bufs;
    w.st = static_cast<hipStream_t>(stream);
    for (const Step& s : dgrad::plan_steps(d)) {
        const int32_t rc = dgrad::run_step(s, w);
        if (rc != M2_OK) return rc;
    }
    return M2_OK;
}

int32_t m2_debug_decoder_grad_plan(int32_t H, int32_t M, int32_t layers, int32_t heads, int32_t B, int32_t T, char* out,
                                   size_t cap) {
    const Dims d{H, M, layers, heads, B, T};
    M2_CHECK_ARG(out && cap > 0 && B > 0 && T > 0, "m2_debug_decoder_grad_plan: bad argument");
    M2_CHECK_SHAPE(dgrad::dims_ok(d), kDimsMsg);
    const std::string line = dgrad::print_plan(d);
    const size_t n = std::min(line.size(), cap - 1);
    std::memcpy(out, line.data(), n);
    out[n] = '\0';
    return (int32_t)line.size();
}

// ---- the kernels alone -------------------------------------------------------------

size_t m2_attention_backward_workspace_bytes(int32_t B, int32_t N, int32_t heads) {
    if (B <= 0 || N <= 0 || heads <= 0) return 0;
    return dgrad::att_stat_floats(B, heads, N) * sizeof(float) + 256;
}

int32_t m2_attention_backward(const float* qkv, const uint8_t* key_mask, const float* att, const float* d_att,
                              int32_t B, int32_t N, int32_t H, int32_t heads, float* d_qkv, void* workspace,
                              size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(qkv && att && d_att && d_qkv && B >= 0 && N >= 0 && H > 0 && heads > 0,
                 "m2_attention_backward: bad argument");
    M2_CHECK_SHAPE(H % heads == 0 && dgrad::head_dim_ok(H / heads) && B <= loss::kMaxGrid && heads <= loss::kMaxGrid &&
                       N <= (1 << 22),
                   "m2_attention_backward: head_dim must be 16, 32, 48 or 64");
    if (B == 0 || N == 0) return M2_OK;
    Carve cv(workspace, workspace_bytes);
    float* stats = cv.take<float>(dgrad::att_stat_floats(B, heads, N));
    if (!cv.ok) return fail(M2_E_ARG, "m2_attention_backward: workspace too small");
    return launch_att_bwd(qkv, key_mask, att, d_att, B, N, H, heads, d_qkv, stats, static_cast<hipStream_t>(stream));
}

size_t m2_linear_backward_input_workspace_bytes(int32_t R, int32_t K) {
    if (R <= 0 || K <= 0) return 0;
    return dgrad::dx_part_floats((size_t)R, K, dgrad::DX_LN) * sizeof(float) + 256;
}

int32_t m2_linear_backward_input(const float* g_y, const float* w, const float* relu_of, const float* ln_x,
                                 const float* gamma, const float* g_res, int32_t R, int32_t K, int32_t N, float* g_x,
                                 float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(g_y && w && R >= 0 && !(relu_of && ln_x) && (ln_x != nullptr) == (gamma != nullptr) &&
                     (ln_x || (!g_res && !dgamma && !dbeta)) && (g_x || dgamma || dbeta),
                 "m2_linear_backward_input: bad argument");
    const DxMode mode = ln_x ? dgrad::DX_LN : relu_of ? dgrad::DX_RELU : dgrad::DX_PLAIN;
    M2_CHECK_SHAPE(dgrad::dx_ok(K, N, mode) && R <= (1 << 24),
                   "m2_linear_backward_input: K a multiple of 8, at most 256 (128 with a LayerNorm)");
    M2_CHECK_ARG(g_x || mode == dgrad::DX_LN, "m2_linear_backward_input: bad argument");
    if (R == 0) return M2_OK;
    float* part = nullptr;
    if (dgamma || dbeta) {
        Carve cv(workspace, workspace_bytes);
        part = cv.take<float>(dgrad::dx_part_floats((size_t)R, K, mode));
        if (!cv.ok) return fail(M2_E_ARG, "m2_linear_backward_input: workspace too small");
    }
    return launch_dx(g_y, w, mode, ln_x ? ln_x : relu_of, gamma, g_res, (size_t)R, K, N, g_x, dgamma, dbeta, false, part,
                     static_cast<hipStream_t>(stream));
}

size_t m2_linear_backward_weight_workspace_bytes(int32_t R, int32_t K, int32_t N) {
    if (R <= 0 || !dgrad::dw_ok(K, N)) return 0;
    return dgrad::dw_split((size_t)R, K, N).part_floats * sizeof(float) + 256;
}

int32_t m2_linear_backward_weight(const float* g_y, const float* x, const float* ln_gamma, const float* ln_beta,
                                  int32_t R, int32_t K, int32_t N, float* dw, float* db, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(g_y && x && (dw || db) && R >= 0 && (ln_gamma == nullptr) == (ln_beta == nullptr),
                 "m2_linear_backward_weight: bad argument");
    M2_CHECK_SHAPE(dgrad::dw_ok(K, N) && R <= (1 << 24), "m2_linear_backward_weight: K a multiple of 8, at most 256");
    if (R == 0) {  // an empty sum
        if (dw) M2_HIP(hipMemsetAsync(dw, 0, (size_t)N * K * sizeof(float), static_cast<hipStream_t>(stream)));
        if (db) M2_HIP(hipMemsetAsync(db, 0, (size_t)N * sizeof(float), static_cast<hipStream_t>(stream)));
        return M2_OK;
    }
    Carve cv(workspace, workspace_bytes);
    float* part = cv.take<float>(dgrad::dw_split((size_t)R, K, N).part_floats);
    if (!cv.ok) return fail(M2_E_ARG, "m2_linear_backward_weight: workspace too small");
    return launch_dw(g_y, x, ln_gamma, ln_beta, (size_t)R, K, N, dw, db, false, part, static_cast<hipStream_t>(stream));
}

}  // extern "C"
