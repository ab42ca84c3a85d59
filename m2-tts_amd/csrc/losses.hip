// Training-loss forward values on the GPU: the sums behind the reference's
// src/training/losses.py (SpectralLoss, PerceptualLoss, MultiScaleDiscriminator,
// AdversarialLoss), batched over utterances.  Forward only: nothing here
// computes a gradient.
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
//   spectral  spectral_frame_kernel: torch.stft framing (centre, reflect
//             padding), pred and target through one complex FFT as in
//             eval_metrics.hip; magnitudes and angles in double from the fp32
//             spectrum; DC and Nyquist imaginary parts are +0.
// Every reduction is a lane-strided sum, an xor-shuffle tree and the wave
// partials in order: no floating-point atomics, equal inputs give equal bits,
// and a batched row equals the row of the utterance run alone.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "audio_dsp.h"

namespace m2 {
namespace loss {

using dsp::block_sum;
using dsp::NT;

struct ConvGeo {
    int Cin, Cout, k, stride, pad, groups;
};

constexpr int kNP = 64;          // output positions per conv_mfma workgroup
constexpr int kCoWg = 64;        // output channels per conv_mfma workgroup (4 waves x 16)
constexpr int kCch = 16;         // input channels staged in LDS per step
constexpr int kMaxLds = 48 * 1024;
constexpr int kMaxGrid = 65535;

constexpr int kLayers = 7;
constexpr int kFeat = 6;         // layers whose output is a feature map (more than one channel)
constexpr int kMaxScales = 8;
const ConvGeo kDisc[kLayers] = {{1, 64, 15, 1, 7, 1},       {64, 128, 41, 4, 20, 4},     {128, 256, 41, 4, 20, 16},
                                {256, 512, 41, 4, 20, 64},  {512, 1024, 41, 4, 20, 256}, {1024, 1024, 5, 1, 2, 1},
                                {1024, 1, 3, 1, 1, 1}};
constexpr float kDiscSlope = 0.2f;

constexpr int kRedChunk = 16384;  // elements per reduce_part_kernel workgroup
constexpr int kRedPart = 4;
constexpr size_t kSliceBytes = (size_t)1 << 30;  // activation bytes a batch slice may take (m2_disc_set_slice_bytes)

constexpr int kSpecPart = 3;  // per frame: sum | |P| - |T| |, sum |angle P - angle T|, the perceptual term
const char* const kSpecCols[] = {"mag_abs", "phase_abs", "bins", "mel_log_abs", "frames"};
constexpr int kSpecK = sizeof(kSpecCols) / sizeof(kSpecCols[0]);
// per scale: logits (5), then per layer (2)
constexpr int kDiscScaleK = 5 + 2 * kFeat;
constexpr int kDiscScales = 3;
constexpr int kDiscK = kDiscScales * kDiscScaleK;

__host__ __device__ inline int conv_out_len(int L, const ConvGeo& g) { return (L + 2 * g.pad - g.k) / g.stride + 1; }
inline int span_of(const ConvGeo& g) { return (kNP - 1) * g.stride + g.k; }
inline int spanp_of(const ConvGeo& g) { return span_of(g) | 1; }

enum Path { PATH_DIRECT = 0, PATH_MFMA = 1, PATH_WAVE = 2 };
inline Path conv_path(const ConvGeo& g) {
    const int K = g.Cin / g.groups * g.k;
    if (g.Cout >= 16 && K >= 32 && (size_t)kCch * spanp_of(g) * sizeof(float) <= (size_t)kMaxLds) return PATH_MFMA;
    return K >= 256 ? PATH_WAVE : PATH_DIRECT;
}

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

// One layer over nb utterances; packed: w is [k, Cin/g, Cout] (MFMA path only).
int32_t launch_conv(const float* x, const float* w, const float* b, float* y, const ConvGeo& g, int nb, int Lraw,
                    int pool, bool packed, float in_slope, float slope, hipStream_t st) {
    const int L = Lraw / pool, Lo = loss::conv_out_len(L, g), Cg = g.Cin / g.groups;
    const loss::Path path = loss::conv_path(g);
    if (pool != 1 && path != loss::PATH_DIRECT) return fail(M2_E_INTERNAL, "launch_conv: only the direct kernel pools");
    if (path == loss::PATH_MFMA) {
        const long long sCo = packed ? 1 : (long long)Cg * g.k, sCi = packed ? g.Cout : g.k,
                        sK = packed ? (long long)Cg * g.Cout : 1;
        const dim3 grid(cdiv(Lo, loss::kNP), cdiv(g.Cout, loss::kCoWg), nb);
        hipLaunchKernelGGL(loss::conv_mfma_kernel, grid, dim3(256), loss::kCch * loss::spanp_of(g) * sizeof(float), st,
                           x, w, b, y, g, L, Lo, sCo, sCi, sK, in_slope, slope);
        M2_LAUNCHED("conv_mfma_kernel");
    } else if (path == loss::PATH_WAVE) {
        hipLaunchKernelGGL(loss::conv_wave_kernel, dim3(cdiv(Lo, 4), g.Cout, nb), dim3(256), 0, st, x, w, b, y, g, L,
                           Lo, in_slope, slope);
        M2_LAUNCHED("conv_wave_kernel");
    } else {
        hipLaunchKernelGGL(loss::conv_direct_kernel, dim3(cdiv(Lo, 256), g.Cout, nb), dim3(256), 0, st, x, w, b, y, g,
                           Lraw, pool, L, Lo, in_slope, slope);
        M2_LAUNCHED("conv_direct_kernel");
    }
    return M2_OK;
}

// Output lengths of the seven layers of the discriminator at `scale`; false when the pooled input is empty.
bool disc_lengths(int L, int scale, int len[kLayers]) {
    int l = L / scale;
    if (l < 1) return false;
    for (int i = 0; i < kLayers; ++i) len[i] = l = loss::conv_out_len(l, kDisc[i]);
    return true;
}

// floats of the seven outputs of one utterance at `scale`
size_t disc_floats(int L, int scale) {
    int len[kLayers];
    if (!disc_lengths(L, scale, len)) return 0;
    size_t n = 0;
    for (int i = 0; i < kLayers; ++i) n += align_up((size_t)kDisc[i].Cout * len[i], 64);
    return n;
}

size_t disc_floats_max(const m2_disc* d, int L) {
    size_t n = 0;
    for (int s = 0; s < d->n_scales; ++s) n = std::max(n, disc_floats(L, d->scales[s]));
    return n;
}

int slice_of(const m2_disc* d, size_t floats_per_utt, int copies, int B) {
    const size_t per = std::max<size_t>(1, floats_per_utt * copies * sizeof(float));
    const size_t n = d->slice_bytes / per;
    return (int)std::max<size_t>(1, std::min<size_t>(n, (size_t)std::max(B, 1)));
}

// The seven layers of scale s over nb utterances of x [nb, 1, L]; out[i] receives layer i.
int32_t run_scale(const m2_disc* d, int s, const float* x, int nb, int L, float* const out[kLayers], hipStream_t st) {
    int Lraw = L, pool = d->scales[s];
    const float* in = x;
    for (int i = 0; i < kLayers; ++i) {
        const bool packed = loss::conv_path(kDisc[i]) == loss::PATH_MFMA;
        const int32_t rc = launch_conv(in, d->w[s][i], d->b[s][i], out[i], kDisc[i], nb, Lraw, pool, packed,
                                       i > 0 ? loss::kDiscSlope : 1.f, 1.f, st);
        if (rc != M2_OK) return rc;
        Lraw = loss::conv_out_len(Lraw / pool, kDisc[i]);
        pool = 1;
        in = out[i];
    }
    return M2_OK;
}

bool disc_shape_ok(const m2_disc* d, int B, int L) {
    if (B > loss::kMaxGrid || L > (1 << 28)) return false;
    for (int s = 0; s < d->n_scales; ++s)
        if (L / d->scales[s] < 1) return false;
    return true;
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
            if (loss::conv_path(g) == loss::PATH_MFMA) {
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
    M2_CHECK_SHAPE(disc_lengths(L, d->scales[scale_index], len), "m2_disc_layer_shape: audio shorter than the scale");
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
                       loss::conv_path(kDisc[layer]) == loss::PATH_MFMA, layer > 0 ? loss::kDiscSlope : 1.f, 1.f,
                       static_cast<hipStream_t>(stream));
}

size_t m2_disc_forward_workspace_bytes(const m2_disc* d, int32_t B, int32_t L) {
    if (!d || B < 0 || L <= 0) return 0;
    const size_t per = disc_floats_max(d, L);
    return (size_t)slice_of(d, per, 1, B) * per * sizeof(float) + 256 * (kLayers + 1);
}

int32_t m2_disc_forward(const m2_disc* d, const float* x, int32_t B, int32_t L, float* logits, float* features,
                        void* workspace, size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(d && x && logits && B >= 0 && L > 0, "m2_disc_forward: bad argument");
    M2_CHECK_SHAPE(disc_shape_ok(d, B, L),
                   "m2_disc_forward: at most 65535 utterances of 2^28 samples, no shorter than the largest scale");
    if (B == 0) return M2_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nbs = slice_of(d, disc_floats_max(d, L), 1, B);
    Carve c(workspace, workspace_bytes);
    float* ws[kLayers];
    {
        int len[kLayers];
        size_t mx[kLayers] = {};
        for (int s = 0; s < d->n_scales; ++s) {
            disc_lengths(L, d->scales[s], len);
            for (int i = 0; i < kLayers; ++i) mx[i] = std::max(mx[i], (size_t)kDisc[i].Cout * len[i]);
        }
        for (int i = 0; i < kLayers; ++i) ws[i] = (features && i < kFeat) || i == kLayers - 1 ? nullptr : c.take<float>(mx[i] * nbs);
        if (!c.ok) return fail(M2_E_WORKSPACE, "m2_disc_forward: workspace too small");
    }
    for (int b0 = 0; b0 < B; b0 += nbs) {
        const int nb = std::min(nbs, B - b0);
        float* lg = logits;
        float* ft = features;
        for (int s = 0; s < d->n_scales; ++s) {
            int len[kLayers];
            disc_lengths(L, d->scales[s], len);
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
    if (!d || B < 0 || L <= 0) return 0;
    const size_t per = disc_floats_max(d, L);
    const int nbs = slice_of(d, per, 2, B);
    const size_t chunks = (size_t)cdiv((int)std::min<size_t>(per, (size_t)1 << 30), loss::kRedChunk) + 1;
    return (size_t)nbs * per * 2 * sizeof(float) + (size_t)nbs * kLayers * chunks * loss::kRedPart * sizeof(double) +
           256 * 4;
}

int32_t m2_disc_losses(const m2_disc* d, const float* real, const float* fake, int32_t B, int32_t L, double* out,
                       void* workspace, size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(d && (real || fake) && out && B >= 0 && L > 0, "m2_disc_losses: bad argument");
    M2_CHECK_SHAPE(d->n_scales == loss::kDiscScales, "m2_disc_losses: the rows are laid out for three scales");
    M2_CHECK_SHAPE(disc_shape_ok(d, B, L),
                   "m2_disc_losses: at most 65535 utterances of 2^28 samples, no shorter than the largest scale");
    if (B == 0) return M2_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t per = disc_floats_max(d, L);
    const int nbs = slice_of(d, per, 2, B);
    const int max_chunks = cdiv((int)std::min<size_t>(per, (size_t)1 << 30), loss::kRedChunk) + 1;
    Carve c(workspace, workspace_bytes);
    float* act[2] = {c.take<float>((size_t)nbs * per), c.take<float>((size_t)nbs * per)};
    double* part = c.take<double>((size_t)nbs * kLayers * max_chunks * loss::kRedPart);
    if (!c.ok) return fail(M2_E_WORKSPACE, "m2_disc_losses: workspace too small");
    for (int b0 = 0; b0 < B; b0 += nbs) {
        const int nb = std::min(nbs, B - b0);
        for (int s = 0; s < d->n_scales; ++s) {
            int len[kLayers];
            disc_lengths(L, d->scales[s], len);
            loss::RedMaps maps;
            int chunks = 1;
            for (int side = 0; side < 2; ++side) {
                const float* x = side ? fake : real;
                float* out_l[kLayers];
                float* p = act[side];
                for (int i = 0; i < kLayers; ++i) {
                    const size_t n = (size_t)kDisc[i].Cout * len[i];
                    out_l[i] = p;
                    (side ? maps.fake : maps.real)[i] = x ? p : nullptr;
                    maps.n[i] = (long long)n;
                    chunks = std::max(chunks, cdiv((int)n, loss::kRedChunk));
                    p += align_up(n, 64) * nb;
                }
                if (!x) continue;
                const int32_t rc = run_scale(d, s, x + (size_t)b0 * L, nb, L, out_l, st);
                if (rc != M2_OK) return rc;
            }
            hipLaunchKernelGGL(loss::reduce_part_kernel, dim3(chunks, kLayers, nb), dim3(dsp::NT), 0, st, maps,
                               max_chunks, part);
            M2_LAUNCHED("reduce_part_kernel");
            hipLaunchKernelGGL(loss::reduce_finish_kernel, dim3(nb), dim3(dsp::NT), 0, st, part, maps, max_chunks,
                               out + (size_t)b0 * loss::kDiscK + (size_t)s * loss::kDiscScaleK, loss::kDiscK);
            M2_LAUNCHED("reduce_finish_kernel");
        }
    }
    return M2_OK;
}

size_t m2_loss_spectral_workspace_bytes(const m2_dsp* d, int32_t B, int32_t L) {
    if (!d || B < 0 || L < 0) return 0;
    return (size_t)B * (1 + L / d->hop) * loss::kSpecPart * sizeof(double) + 256;
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
    double* part = c.take<double>((size_t)B * frames * loss::kSpecPart);
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

}  // extern "C"
