// What the audio kernels share (audio_dsp.hip, eval_metrics.hip, losses.hip):
// the frame workgroup size, the in-LDS FFT, the frame loaders with their
// padding modes, the mel-band and dB bodies that the plain and the ragged
// feature kernels both run, the workgroup reductions and the m2_dsp handle.
#pragma once

#include "m2_common.h"

namespace m2 {
namespace dsp {

constexpr int NT = 256;  // threads per frame workgroup

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// In-LDS radix-2 Stockham FFT of N points (natural order in and out),
// a -> result in a or b (returned).  tw[k] = exp(-2 pi i k / N), k < N/2;
// INV: conjugated twiddles (unnormalised inverse).
template <int N, bool INV>
__device__ float2* fft_lds(float2* a, float2* b, const float2* __restrict__ tw) {
    float2* x = a;
    float2* y = b;
    for (int ns = 1; ns < N; ns <<= 1) {
        for (int j = threadIdx.x; j < N / 2; j += NT) {
            const int k = j & (ns - 1);
            float2 w = tw[k * (N / (2 * ns))];
            if (INV) w.y = -w.y;
            const float2 u = x[j], v = cmul(x[j + N / 2], w);
            const int o = ((j - k) << 1) + k;
            y[o] = make_float2(u.x + v.x, u.y + v.y);
            y[o + ns] = make_float2(u.x - v.x, u.y - v.y);
        }
        __syncthreads();
        float2* t = x;
        x = y;
        y = t;
    }
    return x;
}

// Sample index of a centre-padded frame: i itself inside [0, L); outside, -1
// (a zero sample: librosa pad_mode='constant', the default) or, REFLECT, the
// mirrored index (torch.stft pad_mode='reflect'; needs L > N / 2).
template <bool REFLECT>
__device__ __forceinline__ int pad_index(int i, int L) {
    if (i >= 0 && i < L) return i;
    if (!REFLECT) return -1;
    return i < 0 ? -i : 2 * (L - 1) - i;
}

// Frame t of an utterance whose sample i is fetch(i): samples
// t*hop - N/2 + n (centre padding) times the window, into LDS as complex.
template <int N, bool REFLECT = false, class Fetch>
__device__ __forceinline__ void load_frame_with(Fetch fetch, int L, int hop, int t, const float* __restrict__ win,
                                                float2* a) {
    const int s0 = t * hop - N / 2;
    for (int n = threadIdx.x; n < N; n += NT) {
        const int i = pad_index<REFLECT>(s0 + n, L);
        a[n] = make_float2(i >= 0 ? fetch(i) * win[n] : 0.f, 0.f);
    }
    __syncthreads();
}

// load_frame_with over a float32 signal y[0, L).
template <int N, bool REFLECT = false>
__device__ void load_frame(const float* __restrict__ y, int L, int hop, int t, const float* __restrict__ win, float2* a) {
    load_frame_with<N, REFLECT>([y](int i) { return y[i]; }, L, hop, t, win, a);
}

// load_frame for a pair: pred in the real part, target in the imaginary part.
template <int N, bool REFLECT = false>
__device__ void load_pair_frame(const float* __restrict__ p, const float* __restrict__ q, int L, int hop, int t,
                                const float* __restrict__ win, float2* a) {
    const int s0 = t * hop - N / 2;
    for (int n = threadIdx.x; n < N; n += NT) {
        const int i = pad_index<REFLECT>(s0 + n, L);
        a[n] = make_float2(i >= 0 ? p[i] * win[n] : 0.f, i >= 0 ? q[i] * win[n] : 0.f);
    }
    __syncthreads();
}

// Sum over the workgroup in a fixed order; every thread must call it.
__device__ __forceinline__ double block_sum(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) red[wv] = v;
    __syncthreads();
    v = red[0];
    for (int i = 1; i < nw; ++i) v += red[i];
    return v;
}

// Maximum or minimum over the workgroup (order-independent); every thread
// must call it.
__device__ __forceinline__ float block_reduce(float v, bool is_max, float* red) {
    for (int o = 32; o > 0; o >>= 1) {
        const float w = __shfl_xor(v, o);
        v = is_max ? fmaxf(v, w) : fminf(v, w);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) red[wv] = v;
    __syncthreads();
    v = red[0];
    for (int i = 1; i < nw; ++i) v = is_max ? fmaxf(v, red[i]) : fminf(v, red[i]);
    return v;
}

// The mel branch of an STFT frame: power of the spectrum X (f <= N/2) into
// P, then band m = sum_f W[m, f] P[f] over its bins [lo[m], hi[m]) to
// dst[m * stride].  The plain and the ragged frame kernels both run this.
template <int N>
__device__ __forceinline__ void mel_bands(const float2* X, float* P, const float* __restrict__ W,
                                          const int* __restrict__ lo, const int* __restrict__ hi, int n_mels,
                                          float* __restrict__ dst, size_t stride) {
    constexpr int F = N / 2 + 1;
    for (int f = threadIdx.x; f < F; f += NT) P[f] = X[f].x * X[f].x + X[f].y * X[f].y;
    __syncthreads();
    for (int m = threadIdx.x; m < n_mels; m += NT) {
        float s = 0.f;
        for (int f = lo[m]; f < hi[m]; ++f) s += W[(size_t)m * F + f] * P[f];
        dst[(size_t)m * stride] = s;
    }
}

// power_to_db(ref=max, amin=1e-10, top_db=80) over one utterance's n mel
// powers x, in place, by one workgroup; the floored dB values stay in x and
// the [-1, 1] normalisation of one of them is db_unit(v, lo, sc).
struct DbRange {
    float lo, sc;
};
__device__ __forceinline__ DbRange db_floor(float* __restrict__ x, size_t n, float* red) {
    float mx = -INFINITY;
    for (size_t i = threadIdx.x; i < n; i += blockDim.x) mx = fmaxf(mx, x[i]);
    const float ref = block_reduce(mx, true, red);
    const float off = 10.f * log10f(fmaxf(1e-10f, ref));
    float lmax = -INFINITY;
    for (size_t i = threadIdx.x; i < n; i += blockDim.x) {
        const float v = 10.f * log10f(fmaxf(1e-10f, x[i])) - off;
        x[i] = v;
        lmax = fmaxf(lmax, v);
    }
    const float floor_db = block_reduce(lmax, true, red) - 80.f;
    float vmin = INFINITY, vmax2 = -INFINITY;
    for (size_t i = threadIdx.x; i < n; i += blockDim.x) {
        const float v = fmaxf(x[i], floor_db);
        x[i] = v;
        vmin = fminf(vmin, v);
        vmax2 = fmaxf(vmax2, v);
    }
    const float lo = block_reduce(vmin, false, red), hi = block_reduce(vmax2, true, red);
    return DbRange{lo, 2.f / (hi - lo)};
}
__device__ __forceinline__ float db_unit(float v, DbRange r) { return (v - r.lo) * r.sc - 1.f; }

}  // namespace dsp
}  // namespace m2

// The per-configuration tables (window, twiddles, mel filters and their
// pseudo-inverse) live in one device allocation owned by m2_dsp.
struct m2_dsp {
    int sr, n_fft, hop, win_length, n_mels;
    float fmin, fmax;
    float* buf = nullptr;
    float *win, *W, *Wp;
    float2* tw;
    int *lo, *hi;
    float step;  // NNLS gradient step 1 / ||W||_2^2
};
