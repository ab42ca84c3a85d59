// Training losses on the GPU: the sums behind the reference's
// src/training/losses.py (SpectralLoss, PerceptualLoss, MultiScaleDiscriminator,
// AdversarialLoss), batched over utterances, and three gradients: the
// discriminator loss with respect to the discriminators' parameters, and the
// generator's adversarial and feature-matching terms and its spectral and
// perceptual terms with respect to the audio.
//
//   conv      Conv1d(k, stride, zero padding, groups) + bias, with a leaky
//             slope on the input (the discriminators' feature maps are the
//             convs' outputs before the LeakyReLU, so the next layer's loader
//             applies it) and on the output (the standalone call).  Three
//             kernels chosen by conv_path(): conv_mfma_kernel, an implicit
//             GEMM on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32; tile form,
//             K order and weight layouts at the kernel and in DESIGN 4.6b);
//             conv_direct_kernel, one thread per output (the 1 -> 64 k = 15
//             layer; avg_pool1d fused into its loader); conv_wave_kernel, one
//             wave per output (the 1024 -> 1 k = 3 layer).
//   disc      m2_disc: 3 x 7 layers packed once.  forward walks the batch in
//             slices that bound the workspace (1 GiB of activations by
//             default: the kernels are latency-bound on small grids); losses
//             runs real and fake of a slice scale by scale and reduces logits
//             and feature maps to per-utterance double sums (chunk partials,
//             then one workgroup per utterance) inside the workspace.
//   backward  of y = conv(leaky(x_pre), w) + b, on the same exact-f32 MFMA:
//             conv_dx_mfma_kernel (one stride-1 convolution per stride phase)
//             and conv_dw_mfma_kernel (split over K into partials that
//             dw_finish_kernel adds in order), direct kernels for the rest;
//             m2_disc_step runs each (slice, scale) forward as losses does and
//             then each side backward while its maps are in the workspace,
//             accumulating the 42 gradients in stream order.
//   generator m2_disc_gen_step: the gradient of the adversarial and
//             feature-matching terms with respect to the fake audio.  The
//             forward half again, then the fake side backward with data
//             gradients only: logit_cotangent_kernel, layers 6..1 through the
//             dx kernels above, fm_cotangent_kernel adding the sign term to
//             each map's cotangent before the layer below reads it, and
//             conv_dx_audio_kernel: the first layer's data gradient fused
//             with the adjoint of avg_pool1d and the sum over scales.
//   spectral  spectral_frame_kernel: torch.stft framing (centre, reflect
//             padding), pred and target through one complex FFT as in
//             eval_metrics.hip; magnitudes and angles in double from the fp32
//             spectrum; DC and Nyquist imaginary parts are +0.
//             m2_loss_spectral_backward: spectral_grad_frame_kernel forms the
//             same spectrum, the cotangent of pred's bins in double and its
//             inverse FFT times the window per frame; spectral_fold_kernel
//             gathers the frames and the reflections into each sample.
// Every reduction is a lane-strided sum, an xor-shuffle tree and the wave
// partials in order: no floating-point atomics, equal inputs give equal bits,
// and a batched row equals the row of the utterance run alone.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "audio_dsp.h"
#include "conv_launch.h"
#include "losses_plan.h"

namespace m2 {
namespace loss {

using dsp::block_sum;
using dsp::NT;

constexpr float kDiscSlope = 0.2f;

constexpr int kSpecPart = 3;  // per frame: sum | |P| - |T| |, sum |angle P - angle T|, the perceptual term
const char* const kSpecCols[] = {"mag_abs", "phase_abs", "bins", "mel_log_abs", "frames"};
constexpr int kSpecK = sizeof(kSpecCols) / sizeof(kSpecCols[0]);
// per scale: logits (5), then per layer (2)
constexpr int kDiscScaleK = 5 + 2 * kFeat;
constexpr int kDiscScales = 3;
constexpr int kDiscK = kDiscScales * kDiscScaleK;

__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.f ? v : v * slope; }

typedef float f32x4 __attribute__((ext_vector_type(4)));

// grid (position tiles, channel tiles, utterances); x [nb, Cin, L], y [nb, Cout, Lo].
// Four waves own 64 output channels x 64 positions of one utterance, wave w the
// 16 channels [64 by + 16 w, +16) against four 16-column tiles.  The input
// window of those positions ((64 - 1) stride + k samples per channel) is staged
// in LDS 16 input channels at a time.  K runs tap-major in steps of (tap, 4
// input channels): lane (r, q) = (lane & 15, lane >> 4) supplies
// A = w[co0 + r][ci + q][tap] and B = window[ci + q][(16 t + r) stride + tap].
// A row tile spanning several groups takes the union of their input channels,
// with A = 0 outside a row's own group, and skips the steps outside the union.
// Weight element (co, ci in group, tap) is at w[co sCo + ci sCi + tap sK]:
// PyTorch's [Cout, Cin/g, k], or the handle's packed [k, Cin/g, Cout].
__global__ __launch_bounds__(256) void conv_mfma_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ y,
                                                        ConvGeo g, int L, int Lo, long long sCo, long long sCi,
                                                        long long sK, float in_slope, float slope) {
    extern __shared__ float xs[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
    const int Cg = g.Cin / g.groups, Mg = g.Cout / g.groups;
    const int span = (kNP - 1) * g.stride + g.k, spanp = span | 1;
    const int p0 = blockIdx.x * kNP, cw0 = blockIdx.y * kCoWg, u = blockIdx.z;
    const int cw1 = min(cw0 + kCoWg, g.Cout) - 1;
    const int ciW0 = cw0 / Mg * Cg, ciW1 = (cw1 / Mg + 1) * Cg;  // input channels of this workgroup's groups
    const int co0 = cw0 + wave * 16;
    const bool active = co0 < g.Cout;
    int ca = 0, cb = 0;  // input channels of this wave's groups
    if (active) {
        ca = co0 / Mg * Cg;
        cb = (min(co0 + 15, g.Cout - 1) / Mg + 1) * Cg;
    }
    const int co = co0 + r;
    const bool row = co < g.Cout;
    const int lo = row ? co / Mg * Cg : 0, hi = row ? lo + Cg : 0;
    const float* wrow = w + (row ? (long long)co * sCo : 0);
    const float* xb = x + (size_t)u * g.Cin * L;
    const int nt = min(4, (Lo - p0 + 15) / 16);
    const int i0 = p0 * g.stride - g.pad;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int cs = ciW0; cs < ciW1; cs += kCch) {
        const int nch = min(kCch, ciW1 - cs);
        for (int i = tid; i < nch * span; i += 256) {
            const int c = i / span, o = i - c * span, pos = i0 + o;
            xs[c * spanp + o] = (pos >= 0 && pos < L) ? leaky(xb[(size_t)(cs + c) * L + pos], in_slope) : 0.f;
        }
        __syncthreads();
        if (active) {
            for (int kk = 0; kk < g.k; ++kk) {
                for (int c4 = 0; c4 < nch; c4 += 4) {
                    const int cbase = cs + c4;
                    if (cbase + 4 <= ca || cbase >= cb) continue;  // none of this wave's groups
                    const int ci = cbase + q;
                    const bool v = c4 + q < nch;
                    const float a = (v && ci >= lo && ci < hi) ? wrow[(long long)(ci - lo) * sCi + kk * sK] : 0.f;
                    const float* xr = xs + (c4 + q) * spanp + r * g.stride + kk;
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        if (t < nt) {
                            const float bv = v ? xr[t * 16 * g.stride] : 0.f;
                            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc[t], 0, 0, 0);
                        }
                }
            }
        }
        __syncthreads();
    }
    if (!active) return;
    float* yb = y + (size_t)u * g.Cout * Lo;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = p0 + t * 16 + r;
        if (t < nt && p < Lo) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = co0 + 4 * q + i;
                if (c < g.Cout) yb[(size_t)c * Lo + p] = leaky(acc[t][i] + (bias ? bias[c] : 0.f), slope);
            }
        }
    }
}

// Sample `pos` of channel row xr after avg_pool1d(pool, stride pool): the
// mean of pool raw samples, added in order.
__device__ __forceinline__ float pooled(const float* __restrict__ xr, int pos, int pool) {
    if (pool == 1) return xr[pos];
    float s = 0.f;
    for (int j = 0; j < pool; ++j) s += xr[(size_t)pos * pool + j];
    return s / (float)pool;
}

// grid (position blocks, Cout, utterances); x [nb, Cin, Lraw] read through
// avg_pool1d(pool) to length L = Lraw / pool; PyTorch-layout weights.
__global__ __launch_bounds__(256) void conv_direct_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ y,
                                                          ConvGeo g, int Lraw, int pool, int L, int Lo, float in_slope,
                                                          float slope) {
    const int p = blockIdx.x * 256 + threadIdx.x, co = blockIdx.y, u = blockIdx.z;
    if (p >= Lo) return;
    const int Cg = g.Cin / g.groups, Mg = g.Cout / g.groups;
    const float* xb = x + ((size_t)u * g.Cin + (size_t)(co / Mg) * Cg) * Lraw;
    const float* wr = w + (size_t)co * Cg * g.k;
    float s = 0.f;
    for (int c = 0; c < Cg; ++c)
        for (int kk = 0; kk < g.k; ++kk) {
            const int pos = p * g.stride - g.pad + kk;
            if (pos >= 0 && pos < L)
                s = fmaf(wr[c * g.k + kk], leaky(pooled(xb + (size_t)c * Lraw, pos, pool), in_slope), s);
        }
    y[((size_t)u * g.Cout + co) * Lo + p] = leaky(s + (bias ? bias[co] : 0.f), slope);
}

// grid (cdiv(Lo, 4), Cout, utterances), one wave per output; PyTorch-layout weights.
__global__ __launch_bounds__(256) void conv_wave_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ y,
                                                        ConvGeo g, int L, int Lo, float in_slope, float slope) {
    const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6), co = blockIdx.y, u = blockIdx.z;
    if (p >= Lo) return;
    const int Cg = g.Cin / g.groups, Mg = g.Cout / g.groups, K = Cg * g.k;
    const float* xb = x + ((size_t)u * g.Cin + (size_t)(co / Mg) * Cg) * L;
    const float* wr = w + (size_t)co * K;
    float s = 0.f;
    for (int e = lane; e < K; e += 64) {
        const int c = e / g.k, kk = e - c * g.k, pos = p * g.stride - g.pad + kk;
        if (pos >= 0 && pos < L) s = fmaf(wr[e], leaky(xb[(size_t)c * L + pos], in_slope), s);
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) y[((size_t)u * g.Cout + co) * Lo + p] = leaky(s + (bias ? bias[co] : 0.f), slope);
}

// grid (cdiv(n, 256), B C): y [B, C, L / k] = avg_pool1d(x [B, C, L], k, stride k).
__global__ __launch_bounds__(256) void avg_pool_kernel(const float* __restrict__ x, int L, int k, int Lo,
                                                       float* __restrict__ y) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < Lo) y[(size_t)blockIdx.y * Lo + p] = pooled(x + (size_t)blockIdx.y * L, p, k);
}

// [Cout, Cg, k] -> [k, Cg, Cout]
__global__ __launch_bounds__(256) void pack_weights_kernel(const float* __restrict__ w, int Cout, int Cg, int k,
                                                           float* __restrict__ out) {
    const size_t n = (size_t)Cout * Cg * k;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int co = (int)(i % Cout);
        const size_t rest = i / Cout;
        const int c = (int)(rest % Cg), kk = (int)(rest / Cg);
        out[i] = w[((size_t)co * Cg + c) * k + kk];
    }
}

// grid (chunks, maps, utterances): map m of n[m] elements per utterance at
// real[m] / fake[m] (either may be null).  Feature maps: sum |fake - real|;
// the logits (the last map): sum (real - 1)^2, real^2, (fake - 1)^2, fake^2.
struct RedMaps {
    const float* real[kLayers];
    const float* fake[kLayers];
    long long n[kLayers];
};
__global__ __launch_bounds__(NT) void reduce_part_kernel(RedMaps m, int max_chunks, double* __restrict__ part) {
    __shared__ double red[NT / 64];
    const int c = blockIdx.x, k = blockIdx.y, u = blockIdx.z;
    const long long n = m.n[k], i0 = (long long)c * kRedChunk;
    if (i0 >= n) return;
    const long long i1 = i0 + kRedChunk < n ? i0 + kRedChunk : n;
    const float* rp = m.real[k] ? m.real[k] + (size_t)u * n : nullptr;
    const float* fp = m.fake[k] ? m.fake[k] + (size_t)u * n : nullptr;
    double s[kRedPart] = {0, 0, 0, 0};
    if (k < kFeat) {
        if (rp && fp)
            for (long long i = i0 + threadIdx.x; i < i1; i += NT) s[0] += fabs((double)fp[i] - (double)rp[i]);
    } else {
        for (long long i = i0 + threadIdx.x; i < i1; i += NT) {
            if (rp) {
                const double v = (double)rp[i];
                s[0] += (v - 1.0) * (v - 1.0);
                s[1] += v * v;
            }
            if (fp) {
                const double v = (double)fp[i];
                s[2] += (v - 1.0) * (v - 1.0);
                s[3] += v * v;
            }
        }
    }
    for (int j = 0; j < kRedPart; ++j) s[j] = block_sum(s[j], red);
    if (threadIdx.x == 0) {
        double* o = part + (((size_t)u * kLayers + k) * max_chunks + c) * kRedPart;
        for (int j = 0; j < kRedPart; ++j) o[j] = s[j];
    }
}

// grid (utterances): the columns of one scale of one utterance from the chunk partials.
__global__ __launch_bounds__(NT) void reduce_finish_kernel(const double* __restrict__ part, RedMaps m, int max_chunks,
                                                           double* __restrict__ out, int row_stride) {
    __shared__ double red[NT / 64];
    const int u = blockIdx.x;
    double* o = out + (size_t)u * row_stride;
    for (int k = 0; k < kLayers; ++k) {
        const int chunks = (int)((m.n[k] + kRedChunk - 1) / kRedChunk);
        const double* p = part + ((size_t)u * kLayers + k) * max_chunks * kRedPart;
        double s[kRedPart];
        for (int j = 0; j < kRedPart; ++j) {
            double v = 0.0;
            for (int i = threadIdx.x; i < chunks; i += NT) v += p[(size_t)i * kRedPart + j];
            s[j] = block_sum(v, red);
        }
        if (threadIdx.x == 0) {
            if (k < kFeat) {
                o[5 + 2 * k] = s[0];
                o[5 + 2 * k + 1] = (double)m.n[k];
            } else {
                for (int j = 0; j < kRedPart; ++j) o[j] = s[j];
                o[4] = (double)m.n[k];
            }
        }
    }
}

// ---- backward of y = conv(leaky(x_pre, in_slope), w) + b ---------------------------
// Weight element (co, ci in group, tap) is at w[co sCo + ci sCi + tap sK] as in
// conv_mfma_kernel.  dw and the split-K partials are in PyTorch's [Cout, Cin/g, k].

__device__ __forceinline__ float leaky_grad(float v, float slope) { return v > 0.f ? 1.f : slope; }

// Data gradient.  grid (column tiles, phase blocks x channel tiles, utterances);
// dy [nb, Cout, Lo], x_pre and dx [nb, Cin, L].  Input position u = stride m +
// phase - pad receives the taps phase + stride j against dy[m - j]: one stride-1
// convolution per phase.  The four waves of a workgroup share the columns
// m in [64 bx, +64) and split into pw phases (dx_phases(): 4 from stride 4,
// so that a grouped layer's waves share one staged window) x 4 / pw row tiles
// of 16 input channels: wave w takes phase pw pb + w % pw and the rows
// [16 (4 / pw) tile + 16 (w / pw), +16), by = pb ntile + tile.  K runs over
// (tap j, 4 output channels) with dy's window (64 + J - 1 samples,
// J = ceil(k / stride)) staged in LDS 16 output channels at a time: lane
// (r, q) supplies A = w[co + q][ci0 + r][phase + stride j] and
// B = window[co + q][16 t + r - j].  A row tile spanning several groups takes
// the union of their output channels, A = 0 outside a row's own group.  A
// position no output read gets an empty sum: 0.
__global__ __launch_bounds__(256) void conv_dx_mfma_kernel(const float* __restrict__ x_pre,
                                                           const float* __restrict__ w,
                                                           const float* __restrict__ dy, float* __restrict__ dx,
                                                           ConvGeo g, int L, int Lo, long long sCo, long long sCi,
                                                           long long sK, float in_slope, int J, int pw) {
    extern __shared__ float ds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
    const int Cg = g.Cin / g.groups, Mg = g.Cout / g.groups;
    const int win = kDxM + J - 1, winp = win | 1;
    const int rows = 16 * (4 / pw), ntile = (g.Cin + rows - 1) / rows;  // input channels per workgroup, their tiles
    const int pb = blockIdx.y / ntile, cw0 = (blockIdx.y - pb * ntile) * rows;
    const int m0 = blockIdx.x * kDxM, phase = pb * pw + wave % pw, u = blockIdx.z;
    const int cw1 = min(cw0 + rows, g.Cin) - 1;
    const int coW0 = cw0 / Cg * Mg, coW1 = (cw1 / Cg + 1) * Mg;  // output channels of this workgroup's groups
    const int ci0 = cw0 + wave / pw * 16;
    const bool active = ci0 < g.Cin && phase < g.stride;
    int ca = 0, cb = 0;  // output channels of this wave's groups
    if (active) {
        ca = ci0 / Cg * Mg;
        cb = (min(ci0 + 15, g.Cin - 1) / Cg + 1) * Mg;
    }
    const int ci = ci0 + r;
    const bool row = ci < g.Cin;
    const int grp = row ? ci / Cg : 0;
    const int lo = row ? grp * Mg : 0, hi = row ? lo + Mg : 0;
    const float* wrow = w + (row ? (long long)(ci - grp * Cg) * sCi : 0);
    const float* dyb = dy + (size_t)u * g.Cout * Lo;
    const int M = (L - 1 + g.pad) / g.stride + 1;
    const int nt = min(4, (M - m0 + 15) / 16);
    const int nj = phase < g.k ? (g.k - phase + g.stride - 1) / g.stride : 0;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int cs = coW0; cs < coW1; cs += kCch) {
        const int nch = min(kCch, coW1 - cs);
        for (int i = tid; i < nch * win; i += 256) {
            const int c = i / win, o = i - c * win, t = m0 - (J - 1) + o;
            ds[c * winp + o] = (t >= 0 && t < Lo) ? dyb[(size_t)(cs + c) * Lo + t] : 0.f;
        }
        __syncthreads();
        if (active) {
            for (int j = 0; j < nj; ++j) {
                const long long tapo = (long long)(phase + g.stride * j) * sK;
                for (int c4 = 0; c4 < nch; c4 += 4) {
                    const int cbase = cs + c4;
                    if (cbase + 4 <= ca || cbase >= cb) continue;  // none of this wave's groups
                    const int co = cbase + q;
                    const bool v = c4 + q < nch;
                    const float a = (v && co >= lo && co < hi) ? wrow[(long long)co * sCo + tapo] : 0.f;
                    const float* br = ds + (c4 + q) * winp + r + (J - 1) - j;
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        if (t < nt) {
                            const float bv = v ? br[t * 16] : 0.f;
                            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc[t], 0, 0, 0);
                        }
                }
            }
        }
        __syncthreads();
    }
    if (!active) return;
    const float* xb = x_pre + (size_t)u * g.Cin * L;
    float* dxb = dx + (size_t)u * g.Cin * L;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const long long pos = (long long)(m0 + t * 16 + r) * g.stride + phase - g.pad;
        if (t < nt && pos >= 0 && pos < L) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = ci0 + 4 * q + i;
                if (c < g.Cin) dxb[(size_t)c * L + pos] = acc[t][i] * leaky_grad(xb[(size_t)c * L + pos], in_slope);
            }
        }
    }
}

// Data gradient, one thread per input sample.  grid (position blocks, Cin, utterances).
__global__ __launch_bounds__(256) void conv_dx_direct_kernel(const float* __restrict__ x_pre,
                                                             const float* __restrict__ w,
                                                             const float* __restrict__ dy, float* __restrict__ dx,
                                                             ConvGeo g, int L, int Lo, long long sCo, long long sCi,
                                                             long long sK, float in_slope) {
    const int pos = blockIdx.x * 256 + threadIdx.x, ci = blockIdx.y, u = blockIdx.z;
    if (pos >= L) return;
    const int Cg = g.Cin / g.groups, Mg = g.Cout / g.groups, grp = ci / Cg;
    const float* wr = w + (long long)(ci - grp * Cg) * sCi;
    const float* dyb = dy + ((size_t)u * g.Cout + (size_t)grp * Mg) * Lo;
    const int v = pos + g.pad;
    float s = 0.f;
    for (int c = 0; c < Mg; ++c)
        for (int tap = v % g.stride; tap < g.k && tap <= v; tap += g.stride) {
            const int t = (v - tap) / g.stride;
            if (t < Lo) s = fmaf(wr[(long long)(grp * Mg + c) * sCo + (long long)tap * sK], dyb[(size_t)c * Lo + t], s);
        }
    const size_t i = ((size_t)u * g.Cin + ci) * L + pos;
    dx[i] = s * leaky_grad(x_pre[i], in_slope);
}

// Weight gradient partials.  grid (input-channel blocks, 16-row tiles of output
// channels, splits).  A row tile takes the union of the input channels of the
// groups it touches, nciB at a time; the columns of a workgroup are (input
// channel, tap) pairs numbered c k + tap, 16 to a tile, wave w the tiles
// w, w + 4, ...  K runs over (utterance, output position) in chunks of 64
// positions, split z the chunks [z cps, (z + 1) cps): dy[16][64] and the input
// window of those positions ((64 - 1) stride + k samples per channel, through
// leaky) are staged in LDS; lane (r, q) supplies A = dy[co0 + r][t + q] and
// B = window[c_r][(t + q) stride + tap_r].  Products of a row with a channel
// outside its own group are not written.  part [splits, Cout, Cin/g, k].
__global__ __launch_bounds__(256) void conv_dw_mfma_kernel(const float* __restrict__ x_pre,
                                                           const float* __restrict__ dy, float* __restrict__ part,
                                                           ConvGeo g, int nb, int L, int Lo, float in_slope,
                                                           int nciB, int cps) {
    extern __shared__ float sm[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
    const int Cg = g.Cin / g.groups, Mg = g.Cout / g.groups;
    const int span = (kTc - 1) * g.stride + g.k, spanp = span | 1;
    const int co0 = blockIdx.y * 16;
    const int gA = co0 / Mg, gB = min(co0 + 15, g.Cout - 1) / Mg;
    const int cb0 = blockIdx.x * nciB, U = (gB + 1 - gA) * Cg;
    if (cb0 >= U) return;
    const int c0 = gA * Cg + cb0, nci = min(nciB, U - cb0);
    const int ncols = nci * g.k, ntiles = (ncols + 15) / 16;
    float* xs = sm;
    float* dys = sm + (size_t)nciB * spanp;
    int off[kDwTiles];
#pragma unroll
    for (int i = 0; i < kDwTiles; ++i) {
        const int n = (wave + 4 * i) * 16 + r;
        const int c = n / g.k;
        off[i] = n < ncols ? c * spanp + (n - c * g.k) : 0;
    }
    f32x4 acc[kDwTiles];
#pragma unroll
    for (int i = 0; i < kDwTiles; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int tcn = (Lo + kTc - 1) / kTc, total = nb * tcn;
    const int ch1 = min(total, ((int)blockIdx.z + 1) * cps);
    for (int ch = blockIdx.z * cps; ch < ch1; ++ch) {
        const int b = ch / tcn, t0 = (ch - b * tcn) * kTc, nt = min(kTc, Lo - t0);
        const float* dyb = dy + (size_t)b * g.Cout * Lo;
        for (int i = tid; i < 16 * kTc; i += 256) {
            const int rr = i / kTc, tt = i - rr * kTc;
            dys[rr * (kTc + 1) + tt] = (co0 + rr < g.Cout && tt < nt) ? dyb[(size_t)(co0 + rr) * Lo + t0 + tt] : 0.f;
        }
        const float* xb = x_pre + ((size_t)b * g.Cin + c0) * L;
        const long long i0 = (long long)t0 * g.stride - g.pad;
        for (int i = tid; i < nci * span; i += 256) {
            const int c = i / span, o = i - c * span;
            const long long pos = i0 + o;
            xs[c * spanp + o] = (pos >= 0 && pos < L) ? leaky(xb[(size_t)c * L + pos], in_slope) : 0.f;
        }
        __syncthreads();
        for (int t4 = 0; t4 < nt; t4 += 4) {
            const float a = dys[r * (kTc + 1) + t4 + q];
            const float* xr = xs + (t4 + q) * g.stride;
#pragma unroll
            for (int i = 0; i < kDwTiles; ++i)
                if (wave + 4 * i < ntiles) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xr[off[i]], acc[i], 0, 0, 0);
        }
        __syncthreads();
    }
    float* po = part + (size_t)blockIdx.z * g.Cout * Cg * g.k;
#pragma unroll
    for (int i = 0; i < kDwTiles; ++i) {
        const int n = (wave + 4 * i) * 16 + r;
        if (wave + 4 * i < ntiles && n < ncols) {
            const int c = n / g.k, tap = n - c * g.k, ci = c0 + c, grp = ci / Cg;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int co = co0 + 4 * q + j;
                if (co < g.Cout && co / Mg == grp) po[((size_t)co * Cg + (ci - grp * Cg)) * g.k + tap] = acc[i][j];
            }
        }
    }
}

// dw[i] = (accumulate ? dw[i] : 0) + the partials of i in split order.
__global__ __launch_bounds__(256) void dw_finish_kernel(const float* __restrict__ part, size_t n, int splits,
                                                        int accumulate, float* __restrict__ dw) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = accumulate ? dw[i] : 0.f;
    for (int k = 0; k < splits; ++k) s += part[(size_t)k * n + i];
    dw[i] = s;
}

// Weight gradient, one workgroup per element.  grid (Cout Cin/g k).
__global__ __launch_bounds__(NT) void conv_dw_direct_kernel(const float* __restrict__ x_pre,
                                                            const float* __restrict__ dy, float* __restrict__ dw,
                                                            ConvGeo g, int nb, int L, int Lo, float in_slope,
                                                            int accumulate) {
    __shared__ double red[NT / 64];
    const int Cg = g.Cin / g.groups, Mg = g.Cout / g.groups;
    const int tap = blockIdx.x % g.k, rest = blockIdx.x / g.k, cig = rest % Cg, co = rest / Cg;
    const int ci = co / Mg * Cg + cig;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) {
        const float* xr = x_pre + ((size_t)b * g.Cin + ci) * L;
        const float* dr = dy + ((size_t)b * g.Cout + co) * Lo;
        for (int t = threadIdx.x; t < Lo; t += NT) {
            const long long pos = (long long)t * g.stride + tap - g.pad;
            if (pos >= 0 && pos < L) s += (double)dr[t] * (double)leaky(xr[pos], in_slope);
        }
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) dw[blockIdx.x] = (accumulate ? dw[blockIdx.x] : 0.f) + (float)s;
}

// db[co] = (accumulate ? db[co] : 0) + sum over utterances and positions of dy.  grid (Cout),
// kDbThreads threads: few workgroups (64 on the first layer) each stream a whole channel.
__global__ __launch_bounds__(kDbThreads) void conv_db_kernel(const float* __restrict__ dy, int nb, int Cout, int Lo,
                                                             int accumulate, float* __restrict__ db) {
    __shared__ double red[kDbThreads / 64];
    const int co = blockIdx.x;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) {
        const float* dr = dy + ((size_t)b * Cout + co) * Lo;
        for (int t = threadIdx.x; t < Lo; t += kDbThreads) s += (double)dr[t];
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) db[co] = (accumulate ? db[co] : 0.f) + (float)s;
}

// Cotangent of the logits of one side under L_D: scale (D - target), in double, rounded once.
__global__ __launch_bounds__(256) void logit_cotangent_kernel(const float* __restrict__ logits, size_t n, double target,
                                                              double scale, float* __restrict__ dy) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dy[i] = (float)(((double)logits[i] - target) * scale);
}

// The feature-matching term of one map, added to the cotangent of that map:
// cot[i] += c sign(f_fake[i] - f_real[i]), sign(0) = 0 (torch's l1_loss backward).
__global__ __launch_bounds__(256) void fm_cotangent_kernel(const float* __restrict__ f_fake,
                                                           const float* __restrict__ f_real, size_t n, float c,
                                                           float* __restrict__ cot) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float a = f_fake[i], b = f_real[i];
    if (a != b) cot[i] += a > b ? c : a < b ? -c : a - b;  // unordered: the NaN goes on, as torch's sign does
}

// Data gradient of y = conv(avg_pool1d(x, pool), w) for one input channel and
// stride 1 (the discriminators' first layer), down to the audio samples.
// grid (cdiv(L, 256 pool), utterances); dy [nb, Cout, Lo], w [Cout, 1, k],
// dx [nb, 1, L], Lp = L / pool pooled positions, Lo = Lp + 2 pad - k + 1.  A
// workgroup owns the pooled positions u in [256 bx, +256), one per thread:
// acc = sum over (co, tap), in that order, of w[co][tap] dy[co][u + pad - tap],
// with the weights in LDS and dy's window (256 + k - 1 samples, 0 outside
// [0, Lo)) staged 16 channels at a time at an odd row pitch.  The sums change
// hands in LDS, so that consecutive threads write consecutive samples: sample
// i gets acc[i / pool] / pool, overwritten or, with `accumulate`, added to; the
// samples floor pooling dropped (i >= pool Lp) are zeroed or left alone.
__global__ __launch_bounds__(kAuP) void conv_dx_audio_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                             float* __restrict__ dx, int Cout, int k, int pad, int pool,
                                                             int L, int Lp, int Lo, int accumulate) {
    extern __shared__ float ds[];
    const int tid = threadIdx.x, u0 = blockIdx.x * kAuP;
    const int win = kAuP + k - 1, winp = win | 1;
    float* wl = ds;                 // [Cout][k]
    float* wnd = ds + Cout * k;     // [kCch][winp]
    float acc = 0.f;
    if (u0 < Lp) {  // the same for every thread of the workgroup
        for (int i = tid; i < Cout * k; i += kAuP) wl[i] = w[i];
        const float* dyb = dy + (size_t)blockIdx.y * Cout * Lo;
        const int t0 = u0 + pad - (k - 1);
        for (int cs = 0; cs < Cout; cs += kCch) {
            const int nch = min(kCch, Cout - cs);
            for (int i = tid; i < nch * win; i += kAuP) {
                const int c = i / win, o = i - c * win, t = t0 + o;
                wnd[c * winp + o] = (t >= 0 && t < Lo) ? dyb[(size_t)(cs + c) * Lo + t] : 0.f;
            }
            __syncthreads();
            for (int c = 0; c < nch; ++c) {
                const float* wr = wl + (cs + c) * k;
                const float* br = wnd + c * winp + tid + (k - 1);
                for (int tap = 0; tap < k; ++tap) acc = fmaf(wr[tap], br[-tap], acc);
            }
            __syncthreads();
        }
    }
    wnd[tid] = acc / (float)pool;
    __syncthreads();
    float* dxb = dx + (size_t)blockIdx.y * L;
    for (int j = 0; j < pool; ++j) {
        const int o = j * kAuP + tid;
        const long long i = (long long)u0 * pool + o;
        if (i >= L) break;
        if (u0 + o / pool < Lp)
            dxb[i] = (accumulate ? dxb[i] : 0.f) + wnd[o / pool];
        else if (!accumulate)
            dxb[i] = 0.f;
    }
}

// grid (frames, B): frame t of torch.stft(center=True, pad_mode='reflect') of
// pred and target [B, L]; part [B, frames, kSpecPart]; the spectra
// [B, frames, N/2 + 1] are written when asked for.
template <int N>
__global__ __launch_bounds__(NT) void spectral_frame_kernel(const float* __restrict__ pred,
                                                            const float* __restrict__ target, int L, int hop,
                                                            const float* __restrict__ win,
                                                            const float2* __restrict__ tw,
                                                            const float* __restrict__ mel_w, int n_w,
                                                            double* __restrict__ part, float2* __restrict__ sp,
                                                            float2* __restrict__ st) {
    __shared__ float2 a[N], b[N];
    __shared__ double red[NT / 64];
    constexpr int F = N / 2 + 1;
    const int t = blockIdx.x, u = blockIdx.y, frames = gridDim.x;
    dsp::load_pair_frame<N, true>(pred + (size_t)u * L, target + (size_t)u * L, L, hop, t, win, a);
    const float2* Z = dsp::fft_lds<N, false>(a, b, tw);
    double dm = 0.0, da = 0.0, sP = 0.0, sT = 0.0;
    const size_t o0 = ((size_t)u * frames + t) * F;
    for (int f = threadIdx.x; f < F; f += NT) {
        const float2 zf = Z[f], zn = Z[(N - f) & (N - 1)];
        const bool real_bin = f == 0 || f == N / 2;  // a real FFT's DC and Nyquist bins: imaginary part +0
        const float pr = 0.5f * (zf.x + zn.x), pi = real_bin ? 0.f : 0.5f * (zf.y - zn.y);
        const float tr = 0.5f * (zf.y + zn.y), ti = real_bin ? 0.f : 0.5f * (zn.x - zf.x);
        if (sp) sp[o0 + f] = make_float2(pr, pi);
        if (st) st[o0 + f] = make_float2(tr, ti);
        const double mp = sqrt((double)pr * pr + (double)pi * pi), mt = sqrt((double)tr * tr + (double)ti * ti);
        dm += fabs(mp - mt);
        da += fabs(atan2((double)pi, (double)pr) - atan2((double)ti, (double)tr));
        sP += mp;
        sT += mt;
    }
    dm = block_sum(dm, red);
    da = block_sum(da, red);
    sP = block_sum(sP, red);
    sT = block_sum(sT, red);
    double pc = 0.0;
    for (int j = threadIdx.x; j < n_w; j += NT) {
        const double wj = (double)mel_w[j];
        pc += fabs(log(wj * sP + 1e-8) - log(wj * sT + 1e-8));
    }
    pc = block_sum(pc, red);
    if (threadIdx.x == 0) {
        double* o = part + ((size_t)u * frames + t) * kSpecPart;
        o[0] = dm;
        o[1] = da;
        o[2] = pc;
    }
}

__global__ __launch_bounds__(NT) void spectral_finish_kernel(const double* __restrict__ part, int frames, int F,
                                                             double* __restrict__ out) {
    __shared__ double red[NT / 64];
    const int u = blockIdx.x;
    const double* p = part + (size_t)u * frames * kSpecPart;
    double s[kSpecPart];
    for (int k = 0; k < kSpecPart; ++k) {
        double v = 0.0;
        for (int i = threadIdx.x; i < frames; i += NT) v += p[(size_t)i * kSpecPart + k];
        s[k] = block_sum(v, red);
    }
    if (threadIdx.x == 0) {
        double* o = out + (size_t)u * kSpecK;
        o[0] = s[0];
        o[1] = s[1];
        o[2] = (double)frames * (double)F;
        o[3] = s[2];
        o[4] = (double)frames;
    }
}

__device__ __forceinline__ double sign_of(double v) { return v > 0.0 ? 1.0 : v < 0.0 ? -1.0 : 0.0; }

// grid (frames, B): the cotangent of frame t of pred under
//   c_mag sum | |P| - |T| | + c_ph sum |angle P - angle T| + c_perc sum_j |ln(w_j S_P + 1e-8) - ln(w_j S_T + 1e-8)|,
// the sums spectral_frame_kernel takes, from the same loader and FFT (so the
// spectra, S_P and S_T are that kernel's bit for bit).  g = d/dRe P + i d/dIm P
// per bin, in double, rounded once: (c_mag sign(|P| - |T|) + kappa) P / |P| +
// c_ph sign(angle P - angle T) (-Im P + i Re P) / |P|^2, kappa = c_perc sum_j
// sign(ln .. - ln ..) w_j / (w_j S_P + 1e-8); sign(0) = 0 and g = 0 where
// |P| = 0.  g goes into the buffer the spectrum is not in, zero above N/2, and
// through the unnormalised inverse FFT: fr [B, frames, N] receives
// win[n] Re sum_f g_f e^(+2 pi i f n / N), the frame's cotangent.  cot (or
// null) receives g [B, frames, N/2 + 1].
template <int N>
__global__ __launch_bounds__(NT) void spectral_grad_frame_kernel(const float* __restrict__ pred,
                                                                 const float* __restrict__ target, int L, int hop,
                                                                 const float* __restrict__ win,
                                                                 const float2* __restrict__ tw,
                                                                 const float* __restrict__ mel_w, int n_w, double c_mag,
                                                                 double c_ph, double c_perc, float* __restrict__ fr,
                                                                 float2* __restrict__ cot) {
    __shared__ float2 a[N], b[N];
    __shared__ double red[NT / 64];
    constexpr int F = N / 2 + 1;
    const int t = blockIdx.x, u = blockIdx.y, frames = gridDim.x;
    dsp::load_pair_frame<N, true>(pred + (size_t)u * L, target + (size_t)u * L, L, hop, t, win, a);
    const size_t row = (size_t)u * frames + t;
    // The same windowed samples on both sides: P = T and every sign is 0.  The paired FFT rounds its
    // real and imaginary halves differently, so its two spectra would differ there by rounding residue.
    int differs = 0;
    for (int n = threadIdx.x; n < N; n += NT) differs |= a[n].x != a[n].y;
    if (!__syncthreads_or(differs)) {
        for (int n = threadIdx.x; n < N; n += NT) fr[row * N + n] = 0.f;
        if (cot)
            for (int f = threadIdx.x; f < F; f += NT) cot[row * F + f] = make_float2(0.f, 0.f);
        return;
    }
    float2* Z = dsp::fft_lds<N, false>(a, b, tw);
    float2* G = Z == a ? b : a;
    double sP = 0.0, sT = 0.0;
    for (int f = threadIdx.x; f < F; f += NT) {
        const float2 zf = Z[f], zn = Z[(N - f) & (N - 1)];
        const bool real_bin = f == 0 || f == N / 2;
        const float pr = 0.5f * (zf.x + zn.x), pi = real_bin ? 0.f : 0.5f * (zf.y - zn.y);
        const float tr = 0.5f * (zf.y + zn.y), ti = real_bin ? 0.f : 0.5f * (zn.x - zf.x);
        sP += sqrt((double)pr * pr + (double)pi * pi);
        sT += sqrt((double)tr * tr + (double)ti * ti);
    }
    sP = block_sum(sP, red);
    sT = block_sum(sT, red);
    double kappa = 0.0;
    if (c_perc != 0.0) {  // the same for every thread of the workgroup
        for (int j = threadIdx.x; j < n_w; j += NT) {
            const double wj = (double)mel_w[j];
            kappa += sign_of(log(wj * sP + 1e-8) - log(wj * sT + 1e-8)) * wj / (wj * sP + 1e-8);
        }
        kappa = c_perc * block_sum(kappa, red);
    }
    for (int f = threadIdx.x; f < N; f += NT) {
        float2 g = make_float2(0.f, 0.f);
        if (f < F) {
            const float2 zf = Z[f], zn = Z[(N - f) & (N - 1)];
            const bool real_bin = f == 0 || f == N / 2;
            const float pr = 0.5f * (zf.x + zn.x), pi = real_bin ? 0.f : 0.5f * (zf.y - zn.y);
            const float tr = 0.5f * (zf.y + zn.y), ti = real_bin ? 0.f : 0.5f * (zn.x - zf.x);
            const double mp = sqrt((double)pr * pr + (double)pi * pi), mt = sqrt((double)tr * tr + (double)ti * ti);
            if (mp > 0.0) {
                const double radial = (c_mag * sign_of(mp - mt) + kappa) / mp;
                const double turn =
                    c_ph * sign_of(atan2((double)pi, (double)pr) - atan2((double)ti, (double)tr)) / (mp * mp);
                g = make_float2((float)(radial * pr - turn * pi), (float)(radial * pi + turn * pr));
            }
            if (cot) cot[row * F + f] = g;
        }
        G[f] = g;
    }
    __syncthreads();
    const float2* Y = dsp::fft_lds<N, true>(G, Z, tw);
    float* o = fr + row * N;
    for (int n = threadIdx.x; n < N; n += NT) o[n] = win[n] * Y[n].x;
}

// The adjoint of torch.stft's framing (centre, reflect padding): d_pred [B, L]
// from the frames' cotangents fr [B, frames, N].  grid (cdiv(L, 256), B), one
// thread per sample i.  Padded position p is sample n = p + N/2 - t hop of the
// frames t with 0 <= n < N; sample i gathers positions i, then -i
// (1 <= i <= N/2), then 2 (L - 1) - i (L - 1 - N/2 <= i <= L - 2), the frames
// of each ascending, into one fp32 sum, stored or, with `accumulate`, added to
// what is there as one fp32 addition.  Any hop >= 1.
__global__ __launch_bounds__(256) void spectral_fold_kernel(const float* __restrict__ fr, int N, int hop, int frames,
                                                            int L, int accumulate, float* __restrict__ d_pred) {
    const int i = blockIdx.x * 256 + threadIdx.x, u = blockIdx.y;
    if (i >= L) return;
    const float* fu = fr + (size_t)u * frames * N;
    float s = 0.f;
    for (int k = 0; k < 3; ++k) {
        if (k == 1 && !(i >= 1 && i <= N / 2)) continue;
        if (k == 2 && !(i >= L - 1 - N / 2 && i <= L - 2)) continue;
        const int q = (k == 0 ? i : k == 1 ? -i : 2 * (L - 1) - i) + N / 2;  // in [0, L + N)
        const int t0 = q < N ? 0 : (q - N) / hop + 1, t1 = min(frames - 1, q / hop);
        for (int t = t0; t <= t1; ++t) s += fu[(size_t)t * N + (q - t * hop)];
    }
    float* o = d_pred + (size_t)u * L + i;
    *o = accumulate ? *o + s : s;
}

}  // namespace loss
}  // namespace m2

namespace m2 {
namespace loss {

// The launchers of one layer (conv_launch.h), shared with the vocoder's backward.  Grids and LDS
// bytes are the rows of losses_plan.h.
static dim3 grid_of(const LaunchRow& r) { return dim3(r.gx, r.gy, r.gz); }

int32_t launch_conv(const float* x, const float* w, const float* b, float* y, const ConvGeo& g, int nb, int Lraw,
                    int pool, bool packed, float in_slope, float slope, hipStream_t st) {
    const int L = Lraw / pool, Lo = conv_out_len(L, g);
    const Path path = conv_path(g);
    if (pool != 1 && path != PATH_DIRECT) return fail(M2_E_INTERNAL, "launch_conv: only the direct kernel pools");
    const LaunchRow r = conv_row(g, nb, L);
    if (path == PATH_MFMA) {
        const WStride ws = w_stride(g, packed);
        hipLaunchKernelGGL(conv_mfma_kernel, grid_of(r), dim3(r.threads), r.lds, st, x, w, b, y, g, L, Lo, ws.sCo,
                           ws.sCi, ws.sK, in_slope, slope);
    } else if (path == PATH_WAVE) {
        hipLaunchKernelGGL(conv_wave_kernel, grid_of(r), dim3(r.threads), 0, st, x, w, b, y, g, L, Lo, in_slope, slope);
    } else {
        hipLaunchKernelGGL(conv_direct_kernel, grid_of(r), dim3(r.threads), 0, st, x, w, b, y, g, Lraw, pool, L, Lo,
                           in_slope, slope);
    }
    M2_LAUNCHED(r.kernel);
    return M2_OK;
}

int32_t launch_dw_finish(const float* part, size_t n, int splits, bool accumulate, float* dw, hipStream_t st) {
    hipLaunchKernelGGL(dw_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, n, splits,
                       accumulate ? 1 : 0, dw);
    M2_LAUNCHED("dw_finish_kernel");
    return M2_OK;
}

int32_t launch_conv_db(const float* dy, int nb, int Cout, int Lo, bool accumulate, float* db, hipStream_t st) {
    hipLaunchKernelGGL(conv_db_kernel, dim3(Cout), dim3(kDbThreads), 0, st, dy, nb, Cout, Lo, accumulate ? 1 : 0, db);
    M2_LAUNCHED("conv_db_kernel");
    return M2_OK;
}

int32_t launch_conv_bwd(const float* x_pre, const float* w, const float* dy, const ConvGeo& g, int nb, int L,
                        bool packed, float in_slope, float* dx, float* dw, float* db, bool accumulate, float* part,
                        hipStream_t st) {
    const int Lo = conv_out_len(L, g), Cg = g.Cin / g.groups;
    const size_t n = (size_t)g.Cout * Cg * g.k;
    std::vector<LaunchRow> rows;
    conv_bwd_rows(g, nb, L, dx != nullptr, dw != nullptr, false, rows);
    size_t i = 0;
    if (dx) {
        const WStride ws = w_stride(g, packed);
        const LaunchRow& r = rows[i++];
        if (dx_mfma_ok(g))
            hipLaunchKernelGGL(conv_dx_mfma_kernel, grid_of(r), dim3(r.threads), r.lds, st, x_pre, w, dy, dx, g, L, Lo,
                               ws.sCo, ws.sCi, ws.sK, in_slope, cdiv(g.k, g.stride), dx_phases(g));
        else
            hipLaunchKernelGGL(conv_dx_direct_kernel, grid_of(r), dim3(r.threads), 0, st, x_pre, w, dy, dx, g, L, Lo,
                               ws.sCo, ws.sCi, ws.sK, in_slope);
        M2_LAUNCHED(r.kernel);
    }
    if (dw) {
        const DwPlan p = dw_plan(g, nb, L);
        const LaunchRow& r = rows[i++];
        if (p.mfma) {
            hipLaunchKernelGGL(conv_dw_mfma_kernel, grid_of(r), dim3(r.threads), r.lds, st, x_pre, dy, part, g, nb, L,
                               Lo, in_slope, p.nciB, p.cps);
            M2_LAUNCHED(r.kernel);
            const int32_t rc = launch_dw_finish(part, n, p.splits, accumulate, dw, st);
            if (rc != M2_OK) return rc;
        } else {
            hipLaunchKernelGGL(conv_dw_direct_kernel, grid_of(r), dim3(r.threads), 0, st, x_pre, dy, dw, g, nb, L, Lo,
                               in_slope, accumulate ? 1 : 0);
            M2_LAUNCHED(r.kernel);
        }
    }
    if (db) return launch_conv_db(dy, nb, g.Cout, Lo, accumulate, db, st);
    return M2_OK;
}

}  // namespace loss
}  // namespace m2

// Packed weights of the discriminators of one MultiScaleDiscriminator.
struct m2_disc {
    int n_scales;
    int scales[m2::loss::kMaxScales];
    size_t slice_bytes = m2::loss::kSliceBytes;
    float* buf = nullptr;
    const float* w[m2::loss::kMaxScales][m2::loss::kLayers];
    const float* b[m2::loss::kMaxScales][m2::loss::kLayers];
};

namespace {
using namespace m2;
using loss::ConvGeo;
using loss::kDisc;
using loss::kFeat;
using loss::kLayers;

bool geo_ok(const ConvGeo& g) {
    return g.Cin > 0 && g.Cout > 0 && g.k > 0 && g.stride > 0 && g.pad >= 0 && g.groups > 0 &&
           g.Cin % g.groups == 0 && g.Cout % g.groups == 0;
}

using loss::launch_conv;
using loss::launch_conv_bwd;

// The handle keeps the weights of the layers on the MFMA path packed as [k, Cin/g, Cout].
bool disc_packed(int layer) { return loss::conv_path(kDisc[layer]) == loss::PATH_MFMA; }
float disc_in_slope(int layer) { return layer > 0 ? loss::kDiscSlope : 1.f; }

loss::DiscPlan disc_plan(const m2_disc* d, int B, int L, loss::DiscMode mode) {
    return loss::disc_plan(d->scales, d->n_scales, d->slice_bytes, B, L, mode);
}

size_t disc_bytes(const m2_disc* d, int B, int L, loss::DiscMode mode) {
    if (!d || B < 0 || L <= 0) return 0;
    Sizer s;
    loss::carve_disc(s, disc_plan(d, B, L, mode), nullptr);
    return s.off + 256;
}

// The seven layers of scale s over nb utterances of x [nb, 1, L]; out[i] receives layer i.
int32_t run_scale(const m2_disc* d, int s, const float* x, int nb, int L, float* const out[kLayers], hipStream_t st) {
    int Lraw = L, pool = d->scales[s];
    const float* in = x;
    for (int i = 0; i < kLayers; ++i) {
        const int32_t rc = launch_conv(in, d->w[s][i], d->b[s][i], out[i], kDisc[i], nb, Lraw, pool, disc_packed(i),
                                       disc_in_slope(i), 1.f, st);
        if (rc != M2_OK) return rc;
        Lraw = loss::conv_out_len(Lraw / pool, kDisc[i]);
        pool = 1;
        in = out[i];
    }
    return M2_OK;
}

// ---- backward ----------------------------------------------------------------------

// The forward half of one (slice, scale) of m2_disc_losses, shared with the two steps so that
// their rows are its rows bit for bit: each side that is given runs into act[side] (map[side][i]
// receives where layer i went, null for a side that is not given), then the two reductions write
// the scale's columns of the slice's rows.
int32_t scale_forward(const m2_disc* d, int s, const float* real, const float* fake, int b0, int nb, int L,
                      const int len[kLayers], float* const act[2], double* part, int max_chunks, double* out,
                      float* map[2][kLayers], hipStream_t st) {
    loss::RedMaps maps;
    int chunks = 1;
    for (int side = 0; side < 2; ++side) {
        const float* x = side ? fake : real;
        float* out_l[kLayers];
        float* p = act[side];
        for (int i = 0; i < kLayers; ++i) {
            const size_t n = (size_t)kDisc[i].Cout * len[i];
            out_l[i] = p;
            map[side][i] = x ? p : nullptr;
            (side ? maps.fake : maps.real)[i] = x ? p : nullptr;
            maps.n[i] = (long long)n;
            chunks = std::max(chunks, cdiv((int)n, loss::kRedChunk));
            p += align_up(n, 64) * nb;
        }
        if (!x) continue;
        const int32_t rc = run_scale(d, s, x + (size_t)b0 * L, nb, L, out_l, st);
        if (rc != M2_OK) return rc;
    }
    hipLaunchKernelGGL(loss::reduce_part_kernel, dim3(chunks, kLayers, nb), dim3(dsp::NT), 0, st, maps, max_chunks,
                       part);
    M2_LAUNCHED("reduce_part_kernel");
    hipLaunchKernelGGL(loss::reduce_finish_kernel, dim3(nb), dim3(dsp::NT), 0, st, part, maps, max_chunks,
                       out + (size_t)b0 * loss::kDiscK + (size_t)s * loss::kDiscScaleK, loss::kDiscK);
    M2_LAUNCHED("reduce_finish_kernel");
    return M2_OK;
}

// The first-layer data gradient down to the audio samples (conv_dx_audio_kernel's layout).
int32_t launch_audio_bwd(const float* dy, const float* w, int Cout, int k, int pad, int pool, int nb, int L,
                         bool accumulate, float* dx, hipStream_t st) {
    const int Lp = L / pool, Lo = Lp + 2 * pad - k + 1;
    hipLaunchKernelGGL(loss::conv_dx_audio_kernel, dim3((unsigned)(((long long)L + (long long)loss::kAuP * pool - 1) /
                                                                   ((long long)loss::kAuP * pool)), nb),
                       dim3(loss::kAuP), loss::audio_lds_bytes(Cout, k), st, dy, w, dx, Cout, k, pad, pool, L, Lp, Lo,
                       accumulate ? 1 : 0);
    M2_LAUNCHED("conv_dx_audio_kernel");
    return M2_OK;
}

// One side of scale s backward over the nb utterances of a slice, while its maps are resident:
// the logits' cotangent cscale (D - target), then layers kLayers - 1 .. lowest.  The cotangent of
// a layer's output is in one of bufs.cot and that of its input goes to the other; *last (or null)
// receives the one written last.  Layer i reads map[i - 1], layer 0 reads x0 [nb, 1, L0] and has
// no data gradient.  grads (or null: data gradients only) are the scale's (weight, bias) pairs,
// overwritten or, with `accumulate`, added to.  With w_fm != 0 the feature-matching term of map
// i - 1 against fm_real[i - 1] joins that map's cotangent before the layer below reads it.
int32_t backward_chain(const m2_disc* d, int s, float* const map[kLayers], const float* x0, int L0,
                       const int len[kLayers], int nb, int B, double target, double cscale, int lowest,
                       float* const* grads, bool accumulate, float* const fm_real[kLayers], double w_fm,
                       const loss::DiscBufs& bufs, const float** last, hipStream_t st) {
    const size_t nl = (size_t)nb * len[kLayers - 1];
    hipLaunchKernelGGL(loss::logit_cotangent_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, st,
                       map[kLayers - 1], nl, target, cscale, bufs.cot[0]);
    M2_LAUNCHED("logit_cotangent_kernel");
    int cur = 0;
    for (int i = kLayers - 1; i >= lowest; --i) {
        const int32_t rc = launch_conv_bwd(i > 0 ? map[i - 1] : x0, d->w[s][i], bufs.cot[cur], kDisc[i], nb,
                                           i > 0 ? len[i - 1] : L0, disc_packed(i), disc_in_slope(i),
                                           i > 0 ? bufs.cot[cur ^ 1] : nullptr, grads ? grads[2 * i] : nullptr,
                                           grads ? grads[2 * i + 1] : nullptr, accumulate, bufs.part, st);
        if (rc != M2_OK) return rc;
        cur ^= 1;
        if (i > 0 && w_fm != 0.0) {
            const size_t per_utt = (size_t)kDisc[i - 1].Cout * len[i - 1], n = per_utt * nb;
            const double fm = w_fm / ((double)(d->n_scales * kFeat) * (double)B * (double)per_utt);
            hipLaunchKernelGGL(loss::fm_cotangent_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                               map[i - 1], fm_real[i - 1], n, (float)fm, bufs.cot[cur]);
            M2_LAUNCHED("fm_cotangent_kernel");
        }
    }
    if (last) *last = bufs.cot[cur];
    return M2_OK;
}

bool disc_shape_ok(const m2_disc* d, int B, int L) {
    if (B > loss::kMaxGrid || L > (1 << 28)) return false;
    for (int s = 0; s < d->n_scales; ++s)
        if (L / d->scales[s] < 1) return false;
    return true;
}

// m2_disc_losses, m2_disc_step and m2_disc_gen_step (`who`, after its own argument checks): the
// batch in slices, a slice scale by scale.  Each (slice, scale) runs scale_forward and then, while
// the maps of both sides are in the workspace, the backward of the mode.  The discriminator step:
// each side from its (pooled) audio through all seven layers, the 42 gradients overwritten by the
// first (slice, side) and accumulated in stream order by the later ones.  The generator step: the
// fake side with data gradients only down to layer 1, then the first layer fused with the adjoint
// of the pooling; scale index 0 overwrites the slice's rows of d_fake and the later scales add.
int32_t disc_walk(const m2_disc* d, loss::DiscMode mode, const char* who, const float* real, const float* fake, int B,
                  int L, double w_adv, double w_fm, double* out, float* const* grads, float* d_fake, void* workspace,
                  size_t workspace_bytes, hipStream_t st) {
    const std::string name(who);
    if (d->n_scales != loss::kDiscScales)
        return fail(M2_E_SHAPE, (name + ": the rows are laid out for three scales").c_str());
    if (!disc_shape_ok(d, B, L))
        return fail(M2_E_SHAPE,
                    (name + ": at most 65535 utterances of 2^28 samples, no shorter than the largest scale").c_str());
    if (B == 0) return M2_OK;
    const loss::DiscPlan pl = disc_plan(d, B, L, mode);
    Carve c(workspace, workspace_bytes);
    loss::DiscBufs bufs;
    loss::carve_disc(c, pl, &bufs);
    if (!c.ok) return fail(M2_E_WORKSPACE, (name + ": workspace too small").c_str());
    for (int b0 = 0; b0 < B; b0 += pl.nbs) {
        const int nb = std::min(pl.nbs, B - b0);
        for (int s = 0; s < d->n_scales; ++s) {
            int len[kLayers];
            loss::disc_lengths(L, d->scales[s], len);
            float* map[2][kLayers];
            int32_t rc = scale_forward(d, s, real, fake, b0, nb, L, len, bufs.act, bufs.dpart, pl.max_chunks, out, map,
                                       st);
            if (rc != M2_OK) return rc;
            const int Lp = L / d->scales[s];
            const double logits = (double)B * (double)len[kLayers - 1] * (double)d->n_scales;
            if (mode == loss::DISC_STEP) {
                for (int side = 0; side < 2; ++side) {
                    const float* x = (side ? fake : real) + (size_t)b0 * L;
                    if (d->scales[s] > 1) {
                        hipLaunchKernelGGL(loss::avg_pool_kernel, dim3(cdiv(Lp, 256), nb), dim3(256), 0, st, x, L,
                                           d->scales[s], Lp, bufs.pooled);
                        M2_LAUNCHED("avg_pool_kernel");
                        x = bufs.pooled;
                    }
                    rc = backward_chain(d, s, map[side], x, Lp, len, nb, B, side ? 0.0 : 1.0, 2.0 / logits, 0,
                                        grads + (size_t)s * kLayers * 2, b0 > 0 || side > 0, nullptr, 0.0, bufs,
                                        nullptr, st);
                    if (rc != M2_OK) return rc;
                }
            } else if (mode == loss::DISC_GEN_STEP) {
                const float* dy0;
                rc = backward_chain(d, s, map[1], nullptr, 0, len, nb, B, 1.0, w_adv * 2.0 / logits, 1, nullptr, false,
                                    map[0], w_fm, bufs, &dy0, st);
                if (rc != M2_OK) return rc;
                rc = launch_audio_bwd(dy0, d->w[s][0], kDisc[0].Cout, kDisc[0].k, kDisc[0].pad, d->scales[s], nb, L,
                                      s > 0, d_fake + (size_t)b0 * L, st);
                if (rc != M2_OK) return rc;
            }
        }
    }
    return M2_OK;
}

// m2_loss_spectral's workspace: spectral_frame_kernel's partials, [B, frames, kSpecPart].
template <typename A>
void carve_spectral(A& a, const m2_dsp* d, int B, int L, double** part) {
    double* p = a.template take<double>((size_t)B * (1 + L / d->hop) * loss::kSpecPart);
    if (part) *part = p;
}
}  // namespace

extern "C" {

int32_t m2_loss_column_count(int32_t kind) { return kind == 0 ? loss::kSpecK : kind == 1 ? loss::kDiscK : -1; }

const char* m2_loss_column_name(int32_t kind, int32_t index) {
    if (index < 0 || index >= m2_loss_column_count(kind)) return nullptr;
    if (kind == 0) return loss::kSpecCols[index];
    // s<scale>_real_err_sq = sum (D(real) - 1)^2, _real_sq, _fake_err_sq, _fake_sq, _logits (their count);
    // s<scale>_l<layer>_abs_diff = sum |f_fake - f_real|, _count
    static const std::vector<std::string> names = [] {
        static const char* const logit[5] = {"real_err_sq", "real_sq", "fake_err_sq", "fake_sq", "logits"};
        std::vector<std::string> v;
        for (int s = 0; s < loss::kDiscScales; ++s) {
            for (int c = 0; c < 5; ++c) v.push_back("s" + std::to_string(s) + "_" + logit[c]);
            for (int l = 0; l < kFeat; ++l)
                for (int c = 0; c < 2; ++c)
                    v.push_back("s" + std::to_string(s) + "_l" + std::to_string(l) + (c ? "_count" : "_abs_diff"));
        }
        return v;
    }();
    return names[index].c_str();
}

int32_t m2_conv1d_strided(const float* x, const float* w, const float* b, int32_t ksize, int32_t stride,
                          int32_t padding, int32_t groups, float leaky_slope, int32_t B, int32_t Cin, int32_t Cout,
                          int32_t L, float* y, void* stream) {
    const ConvGeo g{Cin, Cout, ksize, stride, padding, groups};
    M2_CHECK_ARG(x && w && y && B >= 0 && L > 0 && Cin > 0 && Cout > 0 && ksize > 0 && stride > 0 && padding >= 0 &&
                     groups > 0,
                 "m2_conv1d_strided: bad argument");
    M2_CHECK_SHAPE(geo_ok(g), "m2_conv1d_strided: groups must divide both channel counts");
    M2_CHECK_SHAPE((long long)L + 2LL * padding >= ksize, "m2_conv1d_strided: kernel wider than the padded input");
    M2_CHECK_SHAPE(B <= loss::kMaxGrid && Cout <= loss::kMaxGrid && L <= (1 << 28) && ksize <= (1 << 16) &&
                       stride <= (1 << 16) && padding <= (1 << 28),
                   "m2_conv1d_strided: at most 65535 utterances and output channels, 2^28 samples and padding, "
                   "2^16 taps and stride");
    if (B == 0) return M2_OK;
    return launch_conv(x, w, b, y, g, B, L, 1, false, 1.f, leaky_slope, static_cast<hipStream_t>(stream));
}

int32_t m2_avg_pool1d(const float* x, int32_t ksize, int32_t B, int32_t C, int32_t L, float* y, void* stream) {
    M2_CHECK_ARG(x && y && ksize > 0 && B >= 0 && C > 0 && L > 0, "m2_avg_pool1d: bad argument");
    M2_CHECK_SHAPE((long long)B * C <= loss::kMaxGrid, "m2_avg_pool1d: at most 65535 rows");
    const int Lo = L / ksize;
    if (B == 0 || Lo == 0) return M2_OK;
    hipLaunchKernelGGL(loss::avg_pool_kernel, dim3(cdiv(Lo, 256), B * C), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, L, ksize, Lo, y);
    M2_LAUNCHED("avg_pool_kernel");
    return M2_OK;
}

int32_t m2_disc_create(const float* const* weights, int32_t count, const int32_t* scales, int32_t n_scales,
                       void* stream, m2_disc** out) {
    M2_CHECK_ARG(weights && scales && out && n_scales > 0 && n_scales <= loss::kMaxScales &&
                     count == n_scales * 2 * kLayers,
                 "m2_disc_create: bad argument");
    for (int i = 0; i < count; ++i) M2_CHECK_ARG(weights[i], "m2_disc_create: null weight");
    for (int s = 0; s < n_scales; ++s) M2_CHECK_ARG(scales[s] > 0, "m2_disc_create: scale must be positive");
    size_t per = 0;
    for (int i = 0; i < kLayers; ++i) {
        const ConvGeo& g = kDisc[i];
        per += align_up((size_t)g.Cout * (g.Cin / g.groups) * g.k, 64) + align_up((size_t)g.Cout, 64);
    }
    auto* d = new m2_disc();
    d->n_scales = n_scales;
    std::memcpy(d->scales, scales, n_scales * sizeof(int));
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipMalloc(&d->buf, per * n_scales * sizeof(float));
    float* p = d->buf;
    for (int s = 0; s < n_scales && e == hipSuccess; ++s)
        for (int i = 0; i < kLayers && e == hipSuccess; ++i) {
            const ConvGeo& g = kDisc[i];
            const int Cg = g.Cin / g.groups;
            const size_t nw = (size_t)g.Cout * Cg * g.k;
            const float* src = weights[(s * kLayers + i) * 2];
            if (disc_packed(i)) {
                hipLaunchKernelGGL(loss::pack_weights_kernel, dim3((unsigned)std::min<size_t>(1024, (nw + 255) / 256)),
                                   dim3(256), 0, st, src, g.Cout, Cg, g.k, p);
                e = hipGetLastError();
            } else {
                e = hipMemcpyAsync(p, src, nw * sizeof(float), hipMemcpyDeviceToDevice, st);
            }
            d->w[s][i] = p;
            p += align_up(nw, 64);
            if (e == hipSuccess)
                e = hipMemcpyAsync(p, weights[(s * kLayers + i) * 2 + 1], g.Cout * sizeof(float),
                                   hipMemcpyDeviceToDevice, st);
            d->b[s][i] = p;
            p += align_up((size_t)g.Cout, 64);
        }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        if (d->buf) (void)hipFree(d->buf);
        delete d;
        return hip_status(e, "m2_disc_create");
    }
    *out = d;
    return M2_OK;
}

int32_t m2_disc_destroy(m2_disc* d) {
    if (!d) return M2_OK;
    const hipError_t e = hipFree(d->buf);
    delete d;
    return e == hipSuccess ? M2_OK : hip_status(e, "m2_disc_destroy");
}

int32_t m2_disc_set_slice_bytes(m2_disc* d, size_t bytes) {
    M2_CHECK_ARG(d, "m2_disc_set_slice_bytes: bad argument");
    d->slice_bytes = bytes ? bytes : loss::kSliceBytes;
    return M2_OK;
}

int32_t m2_disc_layer_shape(const m2_disc* d, int32_t L, int32_t scale_index, int32_t layer, int32_t* channels,
                            int32_t* length) {
    M2_CHECK_ARG(d && channels && length && L > 0 && scale_index >= 0 && scale_index < d->n_scales && layer >= 0 &&
                     layer < kLayers,
                 "m2_disc_layer_shape: bad argument");
    int len[kLayers];
    M2_CHECK_SHAPE(loss::disc_lengths(L, d->scales[scale_index], len), "m2_disc_layer_shape: audio shorter than the scale");
    *channels = kDisc[layer].Cout;
    *length = len[layer];
    return M2_OK;
}

int32_t m2_disc_layer(const m2_disc* d, int32_t scale_index, int32_t layer, const float* x, int32_t B, int32_t L,
                      float* y, void* stream) {
    M2_CHECK_ARG(d && x && y && B >= 0 && L > 0 && scale_index >= 0 && scale_index < d->n_scales && layer >= 0 &&
                     layer < kLayers,
                 "m2_disc_layer: bad argument");
    M2_CHECK_SHAPE(B <= loss::kMaxGrid && L <= (1 << 28), "m2_disc_layer: at most 65535 utterances of 2^28 samples");
    if (B == 0) return M2_OK;
    return launch_conv(x, d->w[scale_index][layer], d->b[scale_index][layer], y, kDisc[layer], B, L, 1,
                       disc_packed(layer), disc_in_slope(layer), 1.f, static_cast<hipStream_t>(stream));
}

size_t m2_disc_forward_workspace_bytes(const m2_disc* d, int32_t B, int32_t L) {
    return disc_bytes(d, B, L, loss::DISC_FORWARD);
}

int32_t m2_disc_forward(const m2_disc* d, const float* x, int32_t B, int32_t L, float* logits, float* features,
                        void* workspace, size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(d && x && logits && B >= 0 && L > 0, "m2_disc_forward: bad argument");
    M2_CHECK_SHAPE(disc_shape_ok(d, B, L),
                   "m2_disc_forward: at most 65535 utterances of 2^28 samples, no shorter than the largest scale");
    if (B == 0) return M2_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const loss::DiscPlan pl = disc_plan(d, B, L, loss::DISC_FORWARD);
    Carve c(workspace, workspace_bytes);
    loss::DiscBufs bufs;
    loss::carve_disc(c, pl, &bufs);
    if (!c.ok) return fail(M2_E_WORKSPACE, "m2_disc_forward: workspace too small");
    float* ws[kLayers];  // layer i of a slice when the caller does not ask for it: the widest of the scales
    float* p = bufs.act[0];
    for (int i = 0; i < kLayers; ++i) {
        ws[i] = p;
        p += align_up(pl.layer[i], 64) * pl.nbs;
    }
    for (int b0 = 0; b0 < B; b0 += pl.nbs) {
        const int nb = std::min(pl.nbs, B - b0);
        float* lg = logits;
        float* ft = features;
        for (int s = 0; s < d->n_scales; ++s) {
            int len[kLayers];
            loss::disc_lengths(L, d->scales[s], len);
            float* out[kLayers];
            for (int i = 0; i < kLayers; ++i) {
                const size_t n = (size_t)kDisc[i].Cout * len[i];
                if (i == kLayers - 1) {
                    out[i] = lg + (size_t)b0 * n;
                    lg += (size_t)B * n;
                } else if (features) {
                    out[i] = ft + (size_t)b0 * n;
                    ft += (size_t)B * n;
                } else {
                    out[i] = ws[i];
                }
            }
            const int32_t rc = run_scale(d, s, x + (size_t)b0 * L, nb, L, out, st);
            if (rc != M2_OK) return rc;
        }
    }
    return M2_OK;
}

size_t m2_disc_losses_workspace_bytes(const m2_disc* d, int32_t B, int32_t L) {
    return disc_bytes(d, B, L, loss::DISC_LOSSES);
}

int32_t m2_disc_losses(const m2_disc* d, const float* real, const float* fake, int32_t B, int32_t L, double* out,
                       void* workspace, size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(d && (real || fake) && out && B >= 0 && L > 0, "m2_disc_losses: bad argument");
    return disc_walk(d, loss::DISC_LOSSES, "m2_disc_losses", real, fake, B, L, 0.0, 0.0, out, nullptr, nullptr,
                     workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

size_t m2_conv1d_strided_backward_workspace_bytes(int32_t ksize, int32_t stride, int32_t padding, int32_t groups,
                                                  int32_t B, int32_t Cin, int32_t Cout, int32_t L) {
    const ConvGeo g{Cin, Cout, ksize, stride, padding, groups};
    if (B <= 0 || L <= 0 || Cin <= 0 || Cout <= 0 || ksize <= 0 || stride <= 0 || padding < 0 || groups <= 0 ||
        !geo_ok(g) || (long long)L + 2LL * padding < ksize)
        return 0;
    return loss::dw_plan(g, B, L).part_floats * sizeof(float) + 256;
}

int32_t m2_conv1d_strided_backward(const float* x_pre, const float* w, const float* dy, int32_t ksize, int32_t stride,
                                   int32_t padding, int32_t groups, float in_slope, int32_t B, int32_t Cin,
                                   int32_t Cout, int32_t L, float* dx, float* dw, float* db, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    const ConvGeo g{Cin, Cout, ksize, stride, padding, groups};
    M2_CHECK_ARG(x_pre && w && dy && dw && B >= 0 && L > 0 && Cin > 0 && Cout > 0 && ksize > 0 && stride > 0 &&
                     padding >= 0 && groups > 0,
                 "m2_conv1d_strided_backward: bad argument");
    M2_CHECK_SHAPE(geo_ok(g), "m2_conv1d_strided_backward: groups must divide both channel counts");
    M2_CHECK_SHAPE((long long)L + 2LL * padding >= ksize,
                   "m2_conv1d_strided_backward: kernel wider than the padded input");
    M2_CHECK_SHAPE(B <= loss::kMaxGrid && Cout <= loss::kMaxGrid && Cin <= loss::kMaxGrid && L <= (1 << 28) &&
                       ksize <= (1 << 16) && stride <= (1 << 16) && padding <= (1 << 28) &&
                       (long long)Cout * (Cin / groups) * ksize < (1LL << 31),
                   "m2_conv1d_strided_backward: at most 65535 utterances and channels, 2^28 samples and padding, "
                   "2^16 taps and stride, 2^31 weights");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (B == 0) {  // empty sums
        M2_HIP(hipMemsetAsync(dw, 0, (size_t)Cout * (Cin / groups) * ksize * sizeof(float), st));
        if (db) M2_HIP(hipMemsetAsync(db, 0, (size_t)Cout * sizeof(float), st));
        return M2_OK;
    }
    Carve c(workspace, workspace_bytes);
    const size_t pf = loss::dw_plan(g, B, L).part_floats;
    float* part = pf ? c.take<float>(pf) : nullptr;
    if (!c.ok) return fail(M2_E_WORKSPACE, "m2_conv1d_strided_backward: workspace too small");
    return launch_conv_bwd(x_pre, w, dy, g, B, L, false, in_slope, dx, dw, db, false, part, st);
}

size_t m2_disc_step_workspace_bytes(const m2_disc* d, int32_t B, int32_t L) {
    return disc_bytes(d, B, L, loss::DISC_STEP);
}

int32_t m2_disc_step(const m2_disc* d, const float* real, const float* fake, int32_t B, int32_t L, double* out,
                     float* const* grads, void* workspace, size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(d && real && fake && out && grads && B >= 0 && L > 0, "m2_disc_step: bad argument");
    for (int i = 0; i < d->n_scales * 2 * kLayers; ++i) M2_CHECK_ARG(grads[i], "m2_disc_step: null gradient");
    return disc_walk(d, loss::DISC_STEP, "m2_disc_step", real, fake, B, L, 0.0, 0.0, out, grads, nullptr, workspace,
                     workspace_bytes, static_cast<hipStream_t>(stream));
}

int32_t m2_conv1d_audio_backward(const float* dy, const float* w, int32_t ksize, int32_t padding, int32_t pool,
                                 int32_t B, int32_t Cout, int32_t L, int32_t accumulate, float* dx, void* stream) {
    M2_CHECK_ARG(dy && w && dx && ksize > 0 && padding >= 0 && pool > 0 && B >= 0 && Cout > 0 && L > 0,
                 "m2_conv1d_audio_backward: bad argument");
    M2_CHECK_SHAPE(B <= loss::kMaxGrid && L <= (1 << 28) && pool <= (1 << 16) && padding <= (1 << 12) &&
                       loss::audio_bwd_ok(Cout, ksize),
                   "m2_conv1d_audio_backward: at most 65535 utterances of 2^28 samples, pool 2^16, padding 2^12, "
                   "and weights and a 16-channel window that fit LDS");
    M2_CHECK_SHAPE(L / pool + 2 * padding >= ksize && L / pool >= 1,
                   "m2_conv1d_audio_backward: kernel wider than the padded pooled input");
    if (B == 0) return M2_OK;
    return launch_audio_bwd(dy, w, Cout, ksize, padding, pool, B, L, accumulate != 0, dx,
                            static_cast<hipStream_t>(stream));
}

size_t m2_disc_gen_step_workspace_bytes(const m2_disc* d, int32_t B, int32_t L) {
    return disc_bytes(d, B, L, loss::DISC_GEN_STEP);
}

int32_t m2_disc_gen_step(const m2_disc* d, const float* real, const float* fake, int32_t B, int32_t L, double w_adv,
                         double w_fm, double* out, float* d_fake, void* workspace, size_t workspace_bytes,
                         void* stream) {
    M2_CHECK_ARG(d && fake && out && d_fake && B >= 0 && L > 0, "m2_disc_gen_step: bad argument");
    M2_CHECK_ARG(real || w_fm == 0.0, "m2_disc_gen_step: the feature-matching term needs real");
    return disc_walk(d, loss::DISC_GEN_STEP, "m2_disc_gen_step", real, fake, B, L, w_adv, w_fm, out, nullptr, d_fake,
                     workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

size_t m2_loss_spectral_workspace_bytes(const m2_dsp* d, int32_t B, int32_t L) {
    if (!d || B < 0 || L < 0) return 0;
    Sizer s;
    carve_spectral(s, d, B, L, nullptr);
    return s.off + 256;
}

int32_t m2_loss_spectral(const m2_dsp* d, const float* pred, const float* target, int32_t B, int32_t L,
                         const float* mel_weights, int32_t n_weights, double* out, void* spec_pred, void* spec_target,
                         void* workspace, size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(d && pred && target && out && B >= 0 && L > 0 && n_weights >= 0 && (mel_weights || n_weights == 0),
                 "m2_loss_spectral: bad argument");
    M2_CHECK_SHAPE(L > d->n_fft / 2, "m2_loss_spectral: reflect padding needs more than n_fft / 2 samples");
    M2_CHECK_SHAPE(B <= loss::kMaxGrid && L <= (1 << 30), "m2_loss_spectral: at most 65535 utterances of 2^30 samples");
    if (B == 0) return M2_OK;
    const int frames = 1 + L / d->hop;
    Carve c(workspace, workspace_bytes);
    double* part;
    carve_spectral(c, d, B, L, &part);
    if (!c.ok) return fail(M2_E_WORKSPACE, "m2_loss_spectral: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
#define M2_SPEC(NN)                                                                                                  \
    hipLaunchKernelGGL((loss::spectral_frame_kernel<NN>), dim3(frames, B), dim3(dsp::NT), 0, st, pred, target, L,   \
                       d->hop, d->win, d->tw, mel_weights, n_weights, part, static_cast<float2*>(spec_pred),         \
                       static_cast<float2*>(spec_target))
    if (d->n_fft == 512) M2_SPEC(512);
    else if (d->n_fft == 1024) M2_SPEC(1024);
    else M2_SPEC(2048);
#undef M2_SPEC
    M2_LAUNCHED("spectral_frame_kernel");
    hipLaunchKernelGGL(loss::spectral_finish_kernel, dim3(B), dim3(dsp::NT), 0, st, part, frames, d->n_fft / 2 + 1,
                       out);
    M2_LAUNCHED("spectral_finish_kernel");
    return M2_OK;
}

size_t m2_loss_spectral_backward_workspace_bytes(const m2_dsp* d, int32_t B, int32_t L) {
    if (!d || B < 0 || L < 0) return 0;
    Sizer s;
    loss::carve_spectral_bwd(s, d->n_fft, d->hop, B, L, nullptr);
    return s.off + 256;
}

int32_t m2_loss_spectral_backward(const m2_dsp* d, const float* pred, const float* target, int32_t B, int32_t L,
                                  const float* mel_weights, int32_t n_weights, double c_mag, double c_phase,
                                  double c_perc, int32_t accumulate, float* d_pred, void* cot_pred, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(d && pred && target && d_pred && B >= 0 && L > 0 && n_weights >= 0 && (mel_weights || n_weights == 0),
                 "m2_loss_spectral_backward: bad argument");
    M2_CHECK_SHAPE(L > d->n_fft / 2, "m2_loss_spectral_backward: reflect padding needs more than n_fft / 2 samples");
    M2_CHECK_SHAPE(B <= loss::kMaxGrid && L <= (1 << 30),
                   "m2_loss_spectral_backward: at most 65535 utterances of 2^30 samples");
    if (B == 0) return M2_OK;
    const int frames = loss::spectral_frames(L, d->hop);
    Carve c(workspace, workspace_bytes);
    float* fr;
    loss::carve_spectral_bwd(c, d->n_fft, d->hop, B, L, &fr);
    if (!c.ok) return fail(M2_E_WORKSPACE, "m2_loss_spectral_backward: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
#define M2_SPEC_GRAD(NN)                                                                                             \
    hipLaunchKernelGGL((loss::spectral_grad_frame_kernel<NN>), dim3(frames, B), dim3(dsp::NT), 0, st, pred, target, \
                       L, d->hop, d->win, d->tw, mel_weights, n_weights, c_mag, c_phase, c_perc, fr,                 \
                       static_cast<float2*>(cot_pred))
    if (d->n_fft == 512) M2_SPEC_GRAD(512);
    else if (d->n_fft == 1024) M2_SPEC_GRAD(1024);
    else M2_SPEC_GRAD(2048);
#undef M2_SPEC_GRAD
    M2_LAUNCHED("spectral_grad_frame_kernel");
    hipLaunchKernelGGL(loss::spectral_fold_kernel, dim3(cdiv(L, 256), B), dim3(256), 0, st, fr, d->n_fft, d->hop, frames,
                       L, accumulate ? 1 : 0, d_pred);
    M2_LAUNCHED("spectral_fold_kernel");
    return M2_OK;
}

}  // extern "C"
