// Mel features and Griffin-Lim on the GPU: the
// reference's src/utils/audio.py:45-151 (compute_mel_spectrogram,
// mel_to_audio), which call librosa 0.10 (STFT with a periodic Hann window,
// centre zero padding, Slaney mel filters, power_to_db, NNLS, Griffin-Lim).
//
// STFT / iSTFT frames are one workgroup each: the frame is gathered from the
// signal (coalesced, zero outside it), windowed, and transformed by a
// radix-2 Stockham FFT in LDS (ping-pong complex buffers, twiddles from a
// table computed in double precision on the host).  The STFT is HBM-light:
// a frame reads 4 KB of signal and writes 4 KB of spectrum, ~50 kFLOP, so
// the launch is latency-bound at the frame counts of an utterance; it is
// not reshaped into a DFT-GEMM.
//   mel features: frame -> FFT -> |X|^2 -> mel filters (per band a
//     contiguous bin range) -> [n_mels, frames]; then one workgroup per
//     utterance does power_to_db (ref = max, amin 1e-10, top_db 80) and the
//     [-1, 1] normalisation with LDS reductions.
//   ragged mel features: the same two bodies (audio_dsp.h) over utterances
//     of unequal length packed back to back, one workgroup per frame of the
//     whole batch and one per utterance, after a peak pass; PCM16 conversion
//     and peak normalisation are fused into the frame loader, and the padded,
//     truncated, zero-filled [B, n_mels, T_out] is written directly.
//   Griffin-Lim: magnitudes from the mel by projected-gradient NNLS
//     (Nesterov-accelerated, X >= 0, from the clipped pseudo-inverse like
//     librosa.util.nnls's start), then n_iter x [iSTFT frames -> overlap-add
//     with the window-sum-square division -> STFT frames with the momentum
//     update of the phases]; the overlap-add is a gather (each sample sums
//     its <= n_fft / hop frames), so results are deterministic.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "audio_dsp.h"

namespace m2 {
namespace dsp {

// STFT to power, mel filters: mel[b, m, t] = sum_f W[m, f] |X_t[f]|^2
// (band m covers bins [lo[m], hi[m])).  Or the complex spectrum
// spec[b, t, f] (f <= N/2) when spec != null.
template <int N>
__global__ __launch_bounds__(NT) void stft_kernel(const float* __restrict__ y, int L, int hop, int frames,
                                                  const float* __restrict__ win, const float2* __restrict__ tw,
                                                  const float* __restrict__ W, const int* __restrict__ lo,
                                                  const int* __restrict__ hi, int n_mels, float* __restrict__ mel,
                                                  float2* __restrict__ spec) {
    __shared__ float2 a[N], b[N];
    __shared__ float P[N / 2 + 1];
    const int t = blockIdx.x, u = blockIdx.y;
    load_frame<N>(y + (size_t)u * L, L, hop, t, win, a);
    const float2* X = fft_lds<N, false>(a, b, tw);
    if (spec) {
        constexpr int F = N / 2 + 1;
        for (int f = threadIdx.x; f < F; f += NT) spec[((size_t)u * frames + t) * F + f] = X[f];
        return;
    }
    mel_bands<N>(X, P, W, lo, hi, n_mels, mel + (size_t)u * n_mels * frames + t, (size_t)frames);
}

// power_to_db(ref=max, amin=1e-10, top_db=80) and 2 (x - min)/(max - min) - 1,
// in place over one utterance's [n_mels, frames] (one workgroup).
__global__ __launch_bounds__(1024) void db_norm_kernel(float* __restrict__ mel, int n) {
    __shared__ float red[16];
    float* x = mel + (size_t)blockIdx.x * n;
    const DbRange r = db_floor(x, (size_t)n, red);
    for (int i = threadIdx.x; i < n; i += blockDim.x) x[i] = db_unit(x[i], r);
}

// ---- ragged mel features (m2_mel_features_ragged) --------------------------
// Utterance u owns samples [off[u], off[u + 1]) of the packed buffer and
// frames [fp[u], fp[u + 1]) of the batch.  Sample i of it is the float32
// value (int16 PCM: s / 32768) divided by the utterance's peak when one is
// given (pk > 0), exactly the host arithmetic of load_audio(normalize=True).
struct RaggedSamples {
    const void* p;
    int fmt;  // M2_SAMPLES_F32 / M2_SAMPLES_I16
    __device__ __forceinline__ float raw(int64_t i) const {
        return fmt == M2_SAMPLES_I16 ? (float)static_cast<const int16_t*>(p)[i] / 32768.f
                                     : static_cast<const float*>(p)[i];
    }
};

// The largest u in [0, B) with pre[u] <= g, for a non-decreasing pre[0..B]
// with pre[0] <= g < pre[B].
__device__ __forceinline__ int ragged_find(const int64_t* __restrict__ pre, int B, int64_t g) {
    int lo = 0, hi = B;  // pre[lo] <= g < pre[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (pre[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Frame prefix fp[0..B] (fp[u + 1] - fp[u] = 1 + L_u / hop) from the sample
// offsets, the stored frame counts, and the peaks cleared; one workgroup.
constexpr int kPrepNT = 1024;
__global__ __launch_bounds__(kPrepNT) void ragged_prep_kernel(const int64_t* __restrict__ off, int B, int hop,
                                                               int max_frames, int64_t* __restrict__ fp,
                                                               unsigned* __restrict__ peak,
                                                               int32_t* __restrict__ out_frames) {
    __shared__ int64_t part[kPrepNT];
    const int per = (B + kPrepNT - 1) / kPrepNT;
    const int u0 = min(B, (int)threadIdx.x * per), u1 = min(B, u0 + per);
    int64_t s = 0;
    for (int u = u0; u < u1; ++u) s += 1 + (off[u + 1] - off[u]) / hop;
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t acc = 0;
        for (int i = 0; i < kPrepNT; ++i) {
            const int64_t v = part[i];
            part[i] = acc;
            acc += v;
        }
        fp[B] = acc;
    }
    __syncthreads();
    s = part[threadIdx.x];
    for (int u = u0; u < u1; ++u) {
        const int64_t T = 1 + (off[u + 1] - off[u]) / hop;
        fp[u] = s;
        s += T;
        peak[u] = 0u;
        out_frames[u] = (int32_t)(max_frames > 0 && T > max_frames ? max_frames : T);
    }
}

// max |x| over the packed samples [s0, s1), strided over the workgroup (the
// partial maxima stay per thread).  With a 16-byte aligned buffer the whole
// 16-byte vectors inside the range are loaded as such.
__device__ __forceinline__ float ragged_range_max(const RaggedSamples& smp, int64_t s0, int64_t s1) {
    float mx = 0.f;
    int64_t a0 = s1, a1 = s1;  // vectors cover [a0, a1)
    if ((reinterpret_cast<uintptr_t>(smp.p) & 15) == 0) {
        const int per = smp.fmt == M2_SAMPLES_I16 ? 8 : 4;
        a0 = min(s1, (s0 + per - 1) / per * per);
        a1 = max(a0, s1 / per * per);
        const int nv = (int)((a1 - a0) / per);
        if (smp.fmt == M2_SAMPLES_I16) {
            const int4* v = reinterpret_cast<const int4*>(static_cast<const int16_t*>(smp.p) + a0);
            for (int k = threadIdx.x; k < nv; k += NT) {
                const int4 q = v[k];
                const int w[4] = {q.x, q.y, q.z, q.w};
                for (int j = 0; j < 4; ++j) {
                    mx = fmaxf(mx, fabsf((float)(int16_t)(w[j] & 0xffff) / 32768.f));
                    mx = fmaxf(mx, fabsf((float)(int16_t)(w[j] >> 16) / 32768.f));
                }
            }
        } else {
            const float4* v = reinterpret_cast<const float4*>(static_cast<const float*>(smp.p) + a0);
            for (int k = threadIdx.x; k < nv; k += NT) {
                const float4 q = v[k];
                mx = fmaxf(fmaxf(fmaxf(mx, fabsf(q.x)), fmaxf(fabsf(q.y), fabsf(q.z))), fabsf(q.w));
            }
        }
    }
    for (int64_t i = s0 + threadIdx.x; i < a0; i += NT) mx = fmaxf(mx, fabsf(smp.raw(i)));
    for (int64_t i = a1 + threadIdx.x; i < s1; i += NT) mx = fmaxf(mx, fabsf(smp.raw(i)));
    return mx;
}

// peak[u] = bits of max |x| over utterance u: a max does not depend on the
// order, and the bits of non-negative floats order as unsigned integers, so
// the integer atomicMax is reproducible.  Each workgroup takes kPeakChunk
// packed samples and walks the utterances that have samples in them (one,
// sometimes two): per utterance a workgroup maximum and one atomic.
constexpr int kPeakChunk = 16384;
__global__ __launch_bounds__(NT) void ragged_peak_kernel(RaggedSamples smp, const int64_t* __restrict__ off, int B,
                                                         unsigned* __restrict__ peak) {
    __shared__ float red[NT / 64];
    const int64_t c0 = (int64_t)blockIdx.x * kPeakChunk, c1 = min(c0 + (int64_t)kPeakChunk, off[B]);
    int64_t s0 = c0;
    for (int u = ragged_find(off, B, c0); s0 < c1; ++u) {  // uniform over the workgroup; ends with u < B
        const int64_t s1 = min(c1, off[u + 1]);
        const float mx = block_reduce(ragged_range_max(smp, s0, s1), true, red);
        if (threadIdx.x == 0) atomicMax(peak + u, __float_as_uint(mx));
        s0 = s1;
    }
}

// One workgroup per frame of the whole batch: stft_kernel's mel branch, the
// conversion and the division by the peak fused into the frame loader.
// raw[n_mels * fp[u] + m * T_u + t]: utterance u's [n_mels, T_u] mel powers.
template <int N>
__global__ __launch_bounds__(NT) void ragged_frame_kernel(RaggedSamples smp, const int64_t* __restrict__ off,
                                                          const int64_t* __restrict__ fp, int B, int hop,
                                                          const unsigned* __restrict__ peak,
                                                          const float* __restrict__ win, const float2* __restrict__ tw,
                                                          const float* __restrict__ W, const int* __restrict__ lo,
                                                          const int* __restrict__ hi, int n_mels,
                                                          float* __restrict__ raw) {
    __shared__ float2 a[N], b[N];
    __shared__ float P[N / 2 + 1];
    const int64_t g = blockIdx.x;
    const int u = ragged_find(fp, B, g);
    const int64_t o = off[u], T = fp[u + 1] - fp[u];
    const int L = (int)(off[u + 1] - o), t = (int)(g - fp[u]);
    const float pk = peak ? __uint_as_float(peak[u]) : 0.f;
    load_frame_with<N>([smp, o, pk](int i) {
        const float v = smp.raw(o + i);
        return pk > 0.f ? v / pk : v;
    }, L, hop, t, win, a);
    const float2* X = fft_lds<N, false>(a, b, tw);
    mel_bands<N>(X, P, W, lo, hi, n_mels, raw + (size_t)n_mels * (size_t)fp[u] + t, (size_t)T);
}

// One workgroup per utterance: db_norm_kernel's arithmetic over all of the
// utterance's frames (in place in raw), then the first out_frames[u] columns
// to out[u, :, :] and exact zeros behind them up to T_out.
__global__ __launch_bounds__(1024) void ragged_db_norm_kernel(float* __restrict__ raw, const int64_t* __restrict__ fp,
                                                              int n_mels, const int32_t* __restrict__ out_frames,
                                                              int T_out, float* __restrict__ out) {
    __shared__ float red[16];
    const int u = blockIdx.x;
    const size_t T = (size_t)(fp[u + 1] - fp[u]);
    float* x = raw + (size_t)n_mels * (size_t)fp[u];
    const DbRange r = db_floor(x, (size_t)n_mels * T, red);
    const size_t keep = (size_t)out_frames[u], To = (size_t)T_out;
    float* y = out + (size_t)u * n_mels * To;
    for (size_t i = threadIdx.x; i < (size_t)n_mels * To; i += blockDim.x) {
        const size_t m = i / To, t = i - m * To;
        y[i] = t < keep ? db_unit(x[m * T + t], r) : 0.f;
    }
}

// Griffin-Lim magnitudes (librosa.feature.inverse.mel_to_stft, power 2):
// X = librosa.util.nnls(W, M) for M = 10^(0.1 (x + 1) / 2), S = sqrt(X).
// librosa solves each block of kNnlsBlockBytes / (n_mels * 4) columns with
// scipy's L-BFGS-B (pgtol 1e-5) on (1 / block size) * 0.5 ||W X - M||^2 from
// X0 = max(0, pinv(W) M), and L-BFGS-B's first act is its convergence test
// at X0: the infinity norm of the projected gradient (g if g < 0, else
// min(x, g)).  For every mel in the reference's normalised range it passes
// (the scaled gradient at X0 is ~1e-7 or less), so librosa returns X0.  Two
// launches reproduce that exactly:
//   nnls_start_kernel  (one workgroup per frame): X0, the residual and the
//     scaled gradient in double, the frame's projected-gradient maximum;
//   nnls_finish_kernel (one per frame): the block's maximum; a converged
//     block stores sqrt(X0) - librosa's result - and a block L-BFGS-B would
//     iterate (mel far outside the normalised range) runs `iters` Nesterov
//     projected-gradient steps per frame from X0 instead, which reaches an
//     NNLS minimiser of the frame but not necessarily L-BFGS-B's (the
//     system is under-determined).
constexpr double kNnlsPgtol = 1e-5;            // scipy fmin_l_bfgs_b default
constexpr int kNnlsBlockBytes = 256 * 1024;    // librosa.util.utils.MAX_MEM_BLOCK
__host__ __device__ inline int nnls_block_cols(int n_mels) {
    const int c = kNnlsBlockBytes / (n_mels * 4);
    return c > 0 ? c : 1;
}

__global__ __launch_bounds__(NT) void nnls_start_kernel(const float* __restrict__ mel, int n_mels, int frames, int F,
                                                        const float* __restrict__ W, const float* __restrict__ Wp,
                                                        float* __restrict__ X0, float* __restrict__ pgmax) {
    extern __shared__ float sh[];
    float* M = sh;                                      // [n_mels]
    float* X = M + n_mels;                              // [F]
    // [n_mels] residual: at float offset n_mels + F rounded up to even (8-B aligned)
    double* r = reinterpret_cast<double*>(sh + ((n_mels + F + 1) & ~1));
    __shared__ double red[NT / 64];
    const int t = blockIdx.x, u = blockIdx.y;
    for (int m = threadIdx.x; m < n_mels; m += NT)
        M[m] = exp10f(0.1f * 0.5f * (mel[((size_t)u * n_mels + m) * frames + t] + 1.f));
    __syncthreads();
    for (int f = threadIdx.x; f < F; f += NT) {
        float s = 0.f;
        for (int m = 0; m < n_mels; ++m) s += Wp[(size_t)f * n_mels + m] * M[m];
        X[f] = fmaxf(s, 0.f);
        X0[((size_t)u * frames + t) * F + f] = X[f];
    }
    __syncthreads();
    for (int m = threadIdx.x; m < n_mels; m += NT) {
        double s = -(double)M[m];
        for (int f = 0; f < F; ++f) s += (double)W[(size_t)m * F + f] * (double)X[f];
        r[m] = s;
    }
    __syncthreads();
    const int bc = nnls_block_cols(n_mels), b0 = t / bc * bc;
    const double inv = 1.0 / ((double)n_mels * (double)min(bc, frames - b0));
    double mx = 0.0;
    for (int f = threadIdx.x; f < F; f += NT) {
        double g = 0.0;
        for (int m = 0; m < n_mels; ++m) g += (double)W[(size_t)m * F + f] * r[m];
        g *= inv;
        const double pg = g < 0.0 ? g : fmin((double)X[f], g);  // L-BFGS-B projgr, bound x >= 0
        mx = fmax(mx, fabs(pg));
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NT / 64; ++w) mx = fmax(mx, red[w]);
        pgmax[(size_t)u * frames + t] = (float)mx;
    }
}

__global__ __launch_bounds__(NT) void nnls_finish_kernel(const float* __restrict__ mel, int n_mels, int frames, int F,
                                                         const float* __restrict__ W, float step, int iters,
                                                         const float* __restrict__ pgmax, float* __restrict__ S) {
    extern __shared__ float sh[];
    float* M = sh;              // [n_mels]
    float* r = M + n_mels;      // [n_mels] residual
    float* X = r + n_mels;      // [F]
    float* Yk = X + F;          // [F] extrapolated point
    __shared__ int conv;
    const int t = blockIdx.x, u = blockIdx.y;
    const int bc = nnls_block_cols(n_mels), b0 = t / bc * bc, b1 = min(frames, b0 + bc);
    float mx = 0.f;
    for (int k = b0 + threadIdx.x; k < b1; k += NT) mx = fmaxf(mx, pgmax[(size_t)u * frames + k]);
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (threadIdx.x == 0) conv = 1;
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && !((double)mx <= kNnlsPgtol)) conv = 0;
    __syncthreads();
    float* srow = S + ((size_t)u * frames + t) * F;  // holds X0 (nnls_start_kernel)
    if (conv || iters == 0) {  // librosa's result: X0
        for (int f = threadIdx.x; f < F; f += NT) srow[f] = sqrtf(srow[f]);
        return;
    }
    for (int m = threadIdx.x; m < n_mels; m += NT)
        M[m] = exp10f(0.1f * 0.5f * (mel[((size_t)u * n_mels + m) * frames + t] + 1.f));
    for (int f = threadIdx.x; f < F; f += NT) {
        X[f] = srow[f];
        Yk[f] = X[f];
    }
    __syncthreads();
    float tk = 1.f;
    for (int it = 0; it < iters; ++it) {
        for (int m = threadIdx.x; m < n_mels; m += NT) {
            float s = -M[m];
            for (int f = 0; f < F; ++f) s += W[(size_t)m * F + f] * Yk[f];
            r[m] = s;
        }
        __syncthreads();
        const float tn = 0.5f * (1.f + sqrtf(1.f + 4.f * tk * tk)), beta = (tk - 1.f) / tn;
        for (int f = threadIdx.x; f < F; f += NT) {
            float g = 0.f;
            for (int m = 0; m < n_mels; ++m) g += W[(size_t)m * F + f] * r[m];
            const float xn = fmaxf(Yk[f] - step * g, 0.f);
            Yk[f] = xn + beta * (xn - X[f]);
            X[f] = xn;
        }
        tk = tn;
        __syncthreads();
    }
    for (int f = threadIdx.x; f < F; f += NT) srow[f] = sqrtf(X[f]);
}

// iSTFT frame t: the spectrum S * angles (Hermitian-completed; the imaginary
// parts of DC and Nyquist dropped, as irfft does), inverse FFT / N, times
// the window -> fr[b, t, 0:N].
template <int N>
__global__ __launch_bounds__(NT) void istft_frame_kernel(const float* __restrict__ S, const float2* __restrict__ ang,
                                                         int frames, const float* __restrict__ win,
                                                         const float2* __restrict__ tw, float* __restrict__ fr) {
    __shared__ float2 a[N], b[N];
    constexpr int F = N / 2 + 1;
    const int t = blockIdx.x, u = blockIdx.y;
    const size_t row = ((size_t)u * frames + t) * F;
    for (int f = threadIdx.x; f < F; f += NT) {
        float2 c = ang[row + f];
        const float m = S[row + f];
        c = make_float2(c.x * m, c.y * m);
        if (f == 0 || f == N / 2) c.y = 0.f;
        a[f] = c;
        if (f > 0 && f < N / 2) a[N - f] = make_float2(c.x, -c.y);
    }
    __syncthreads();
    const float2* x = fft_lds<N, true>(a, b, tw);
    float* o = fr + ((size_t)u * frames + t) * N;
    for (int n = threadIdx.x; n < N; n += NT) o[n] = x[n].x * (1.f / N) * win[n];
}

// Overlap-add with the window-sum-square division (where it exceeds
// tiny(float32)), centre padding trimmed: y[b, i], i < hop (frames - 1).
template <int N>
__global__ __launch_bounds__(256) void ola_kernel(const float* __restrict__ fr, int frames, int hop,
                                                  const float* __restrict__ win, int Lout, float* __restrict__ y) {
    const int i = blockIdx.x * 256 + threadIdx.x, u = blockIdx.y;
    if (i >= Lout) return;
    const int p = i + N / 2;  // position in the untrimmed signal
    int t1 = p / hop;
    if (t1 > frames - 1) t1 = frames - 1;
    const int t0 = p >= N ? (p - N) / hop + 1 : 0;
    float s = 0.f, w2 = 0.f;
    for (int t = t0; t <= t1; ++t) {
        const int n = p - t * hop;
        s += fr[((size_t)u * frames + t) * N + n];
        w2 += win[n] * win[n];
    }
    y[(size_t)u * Lout + i] = w2 > 1.17549435e-38f ? s / w2 : s;
}

// STFT of the rebuilt signal and the Griffin-Lim phase update:
// angles = (X - m/(1+m) prev) / (|.| + tiny), prev = X.
template <int N>
__global__ __launch_bounds__(NT) void gl_update_kernel(const float* __restrict__ y, int L, int hop, int frames,
                                                       const float* __restrict__ win, const float2* __restrict__ tw,
                                                       float mom, float2* __restrict__ ang, float2* __restrict__ prev) {
    __shared__ float2 a[N], b[N];
    constexpr int F = N / 2 + 1;
    const int t = blockIdx.x, u = blockIdx.y;
    load_frame<N>(y + (size_t)u * L, L, hop, t, win, a);
    const float2* X = fft_lds<N, false>(a, b, tw);
    const size_t row = ((size_t)u * frames + t) * F;
    const float c = mom / (1.f + mom);
    for (int f = threadIdx.x; f < F; f += NT) {
        const float2 r = X[f], q = prev[row + f];
        float2 v = make_float2(r.x - c * q.x, r.y - c * q.y);
        const float inv = 1.f / (sqrtf(v.x * v.x + v.y * v.y) + 1.17549435e-38f);
        ang[row + f] = make_float2(v.x * inv, v.y * inv);
        prev[row + f] = r;
    }
}

// y /= max |y| per utterance (audio.py:146-147), one workgroup each.
__global__ __launch_bounds__(1024) void peak_norm_kernel(float* __restrict__ y, int L) {
    __shared__ float red[16];
    float* x = y + (size_t)blockIdx.x * L;
    float mx = 0.f;
    for (int i = threadIdx.x; i < L; i += blockDim.x) mx = fmaxf(mx, fabsf(x[i]));
    mx = block_reduce(mx, true, red);
    if (mx > 0.f)
        for (int i = threadIdx.x; i < L; i += blockDim.x) x[i] /= mx;
}

}  // namespace dsp
}  // namespace m2

// ---------------------------------------------------------------------------
// Host side: the per-configuration tables (window, twiddles, mel filters and
// their pseudo-inverse) live in one device allocation owned by m2_dsp
// (audio_dsp.h).
namespace {
using namespace m2;

double hz_to_mel(double f) {  // librosa Slaney scale
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
double mel_to_hz(double m) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}

// Moore-Penrose pseudo-inverse of the [n_mels x F] filter matrix (full row
// rank): W^T (W W^T)^-1 by Gauss-Jordan on the small n_mels x n_mels Gram
// matrix, in double.
bool pinv_rows(const std::vector<double>& W, int R, int F, std::vector<double>* out) {
    std::vector<double> G((size_t)R * 2 * R, 0.0);
    for (int i = 0; i < R; ++i) {
        for (int j = 0; j < R; ++j) {
            double s = 0.0;
            for (int f = 0; f < F; ++f) s += W[(size_t)i * F + f] * W[(size_t)j * F + f];
            G[(size_t)i * 2 * R + j] = s;
        }
        G[(size_t)i * 2 * R + R + i] = 1.0;
    }
    for (int c = 0; c < R; ++c) {
        int p = c;
        for (int i = c + 1; i < R; ++i)
            if (std::fabs(G[(size_t)i * 2 * R + c]) > std::fabs(G[(size_t)p * 2 * R + c])) p = i;
        if (std::fabs(G[(size_t)p * 2 * R + c]) < 1e-300) return false;
        for (int k = 0; k < 2 * R; ++k) std::swap(G[(size_t)c * 2 * R + k], G[(size_t)p * 2 * R + k]);
        const double d = G[(size_t)c * 2 * R + c];
        for (int k = 0; k < 2 * R; ++k) G[(size_t)c * 2 * R + k] /= d;
        for (int i = 0; i < R; ++i)
            if (i != c) {
                const double e = G[(size_t)i * 2 * R + c];
                if (e != 0.0)
                    for (int k = 0; k < 2 * R; ++k) G[(size_t)i * 2 * R + k] -= e * G[(size_t)c * 2 * R + k];
            }
    }
    out->assign((size_t)F * R, 0.0);  // [F][R] = W^T Ginv
    for (int f = 0; f < F; ++f)
        for (int j = 0; j < R; ++j) {
            double s = 0.0;
            for (int i = 0; i < R; ++i) s += W[(size_t)i * F + f] * G[(size_t)i * 2 * R + R + j];
            (*out)[(size_t)f * R + j] = s;
        }
    return true;
}

int frames_of(const m2_dsp* d, int L) { return 1 + L / d->hop; }  // 1 + (L + 2 (n_fft/2) - n_fft) / hop

// X = librosa.util.nnls(W, M) -> S = sqrt(X) [B, T, F] (nnls_start_kernel /
// nnls_finish_kernel); pg: B * T floats of scratch.
int32_t nnls_magnitudes(const m2_dsp* d, const float* mel, int B, int T, int iters, float* S, float* pg,
                        hipStream_t st) {
    const int F = d->n_fft / 2 + 1;
    const dim3 grid(T, B);
    // M [n_mels] | X [F] floats, rounded up to an even count, then r [n_mels] doubles
    const size_t shs = (((size_t)d->n_mels + (size_t)F + 1) & ~(size_t)1) * sizeof(float) + (size_t)d->n_mels * sizeof(double);
    hipLaunchKernelGGL(dsp::nnls_start_kernel, grid, dim3(dsp::NT), shs, st, mel, d->n_mels, T, F, d->W, d->Wp, S, pg);
    M2_LAUNCHED("nnls_start_kernel");
    const size_t shf = (2 * (size_t)d->n_mels + 2 * (size_t)F) * sizeof(float);
    hipLaunchKernelGGL(dsp::nnls_finish_kernel, grid, dim3(dsp::NT), shf, st, mel, d->n_mels, T, F, d->W, d->step,
                       iters, pg, S);
    M2_LAUNCHED("nnls_finish_kernel");
    return M2_OK;
}

// The workspace layouts, each written once: over a Sizer for the _workspace_bytes function, over
// a Carve for the call.

// m2_mel_features_ragged; the frames of the whole batch are at most B + total_samples / hop.
struct RaggedBufs {
    int64_t* fp;     // frame prefix
    unsigned* peak;  // peaks (float bits)
    float* raw;      // mel powers
};
template <typename A>
void carve_ragged(A& a, const m2_dsp* d, int B, int64_t total_samples, RaggedBufs* out) {
    int64_t* fp = a.template take<int64_t>((size_t)B + 1);
    unsigned* peak = a.template take<unsigned>((size_t)B);
    float* raw = a.template take<float>((size_t)d->n_mels * ((size_t)B + (size_t)(total_samples / d->hop)));
    if (out) *out = RaggedBufs{fp, peak, raw};
}

// nnls_magnitudes' scratch: per-frame projected-gradient maxima.
template <typename A>
void carve_nnls(A& a, int B, int T, float** pg) {
    float* p = a.template take<float>((size_t)B * T);
    if (pg) *pg = p;
}

// m2_griffin_lim; the NNLS scratch is counted whether the magnitudes come from mel or are given.
struct GriffinLimBufs {
    float* S;      // magnitudes
    float2* ang;   // angles
    float2* prev;  // previous rebuilt spectrum
    float* fr;     // windowed inverse frames
    float* y;      // the signal of each iteration
    float* pg;
};
template <typename A>
void carve_griffin_lim(A& a, const m2_dsp* d, int B, int T, GriffinLimBufs* out) {
    const size_t F = d->n_fft / 2 + 1, Lout = (size_t)d->hop * (T > 0 ? T - 1 : 0);
    GriffinLimBufs b;
    b.S = a.template take<float>((size_t)B * T * F);
    b.ang = a.template take<float2>((size_t)B * T * F);
    b.prev = a.template take<float2>((size_t)B * T * F);
    b.fr = a.template take<float>((size_t)B * T * d->n_fft);
    b.y = a.template take<float>((size_t)B * std::max<size_t>(Lout, 1));
    carve_nnls(a, B, T, &b.pg);
    if (out) *out = b;
}
}  // namespace

extern "C" {

int32_t m2_dsp_create(int32_t sample_rate, int32_t n_fft, int32_t hop_length, int32_t win_length, int32_t n_mels,
                      float fmin, float fmax, void* stream, m2_dsp** out) {
    M2_CHECK_ARG(out && sample_rate > 0 && hop_length > 0 && n_mels > 0 && win_length > 0 && win_length <= n_fft &&
                     fmax > fmin && fmin >= 0,
                 "m2_dsp_create: bad argument");
    M2_CHECK_SHAPE(n_fft == 512 || n_fft == 1024 || n_fft == 2048, "m2_dsp_create: n_fft must be 512, 1024 or 2048");
    const int F = n_fft / 2 + 1;
    // periodic Hann of win_length, centred in n_fft (librosa pad_center)
    std::vector<float> win(n_fft, 0.f);
    const int lpad = (n_fft - win_length) / 2;
    for (int k = 0; k < win_length; ++k) win[lpad + k] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * k / win_length));
    std::vector<float> tw(n_fft);  // n_fft/2 complex
    for (int k = 0; k < n_fft / 2; ++k) {
        tw[2 * k] = (float)std::cos(-2.0 * M_PI * k / n_fft);
        tw[2 * k + 1] = (float)std::sin(-2.0 * M_PI * k / n_fft);
    }
    // Slaney mel filters with area normalisation (librosa.filters.mel, htk=False, norm='slaney')
    std::vector<double> mel_f(n_mels + 2);
    const double m0 = hz_to_mel(fmin), m1 = hz_to_mel(fmax);
    for (int i = 0; i < n_mels + 2; ++i) mel_f[i] = mel_to_hz(m0 + (m1 - m0) * i / (n_mels + 1));
    std::vector<double> Wd((size_t)n_mels * F, 0.0);
    std::vector<int> lo(n_mels, F), hi(n_mels, 0);
    for (int i = 0; i < n_mels; ++i) {
        const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
        for (int f = 0; f < F; ++f) {
            const double hz = (double)f * sample_rate / n_fft;
            const double lower = (hz - mel_f[i]) / (mel_f[i + 1] - mel_f[i]);
            const double upper = (mel_f[i + 2] - hz) / (mel_f[i + 2] - mel_f[i + 1]);
            const double w = std::max(0.0, std::min(lower, upper)) * enorm;
            Wd[(size_t)i * F + f] = (double)(float)w;
            if (w > 0) {
                lo[i] = std::min(lo[i], f);
                hi[i] = std::max(hi[i], f + 1);
            }
        }
        if (hi[i] < lo[i]) lo[i] = hi[i] = 0;
    }
    std::vector<double> Pd;
    M2_CHECK_SHAPE(pinv_rows(Wd, n_mels, F, &Pd), "m2_dsp_create: mel filter matrix is rank deficient");
    // ||W||_2^2 = largest eigenvalue of W W^T (power iteration)
    std::vector<double> v(n_mels, 1.0), wv(F), nv(n_mels);
    double lam = 0.0;
    for (int it = 0; it < 200; ++it) {
        for (int f = 0; f < F; ++f) {
            double s = 0.0;
            for (int i = 0; i < n_mels; ++i) s += Wd[(size_t)i * F + f] * v[i];
            wv[f] = s;
        }
        double nrm = 0.0;
        for (int i = 0; i < n_mels; ++i) {
            double s = 0.0;
            for (int f = 0; f < F; ++f) s += Wd[(size_t)i * F + f] * wv[f];
            nv[i] = s;
            nrm += s * s;
        }
        nrm = std::sqrt(nrm);
        lam = nrm;
        for (int i = 0; i < n_mels; ++i) v[i] = nv[i] / nrm;
    }
    auto* d = new m2_dsp();
    d->sr = sample_rate;
    d->n_fft = n_fft;
    d->hop = hop_length;
    d->win_length = win_length;
    d->n_mels = n_mels;
    d->fmin = fmin;
    d->fmax = fmax;
    d->step = (float)(1.0 / lam);
    const size_t nw = n_fft, ntw = n_fft, nW = (size_t)n_mels * F, nP = (size_t)F * n_mels, nl = 2 * (size_t)n_mels;
    std::vector<float> host(nw + ntw + nW + nP + nl, 0.f);
    std::copy(win.begin(), win.end(), host.begin());
    std::copy(tw.begin(), tw.end(), host.begin() + nw);
    for (size_t i = 0; i < nW; ++i) host[nw + ntw + i] = (float)Wd[i];
    for (size_t i = 0; i < nP; ++i) host[nw + ntw + nW + i] = (float)Pd[i];
    std::memcpy(&host[nw + ntw + nW + nP], lo.data(), n_mels * sizeof(int));
    std::memcpy(&host[nw + ntw + nW + nP + n_mels], hi.data(), n_mels * sizeof(int));
    hipError_t e = hipMalloc(&d->buf, host.size() * sizeof(float));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d->buf, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        if (d->buf) (void)hipFree(d->buf);
        delete d;
        return hip_status(e, "m2_dsp_create: upload");
    }
    d->win = d->buf;
    d->tw = reinterpret_cast<float2*>(d->buf + nw);
    d->W = d->buf + nw + ntw;
    d->Wp = d->W + nW;
    d->lo = reinterpret_cast<int*>(d->Wp + nP);
    d->hi = d->lo + n_mels;
    *out = d;
    return M2_OK;
}

int32_t m2_dsp_destroy(m2_dsp* d) {
    if (!d) return M2_OK;
    const hipError_t e = hipFree(d->buf);
    delete d;
    return e == hipSuccess ? M2_OK : hip_status(e, "m2_dsp_destroy");
}

int32_t m2_dsp_frames(const m2_dsp* d, int32_t L) { return d && L >= 0 ? frames_of(d, L) : -1; }

int32_t m2_stft(const m2_dsp* d, const float* audio, int32_t B, int32_t L, void* out_spec, void* stream) {
    M2_CHECK_ARG(d && B >= 0 && L > 0 && (B == 0 || (audio && out_spec)), "m2_stft: bad argument");
    if (B == 0) return M2_OK;
    const int T = frames_of(d, L);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(T, B);
#define M2_STFT(NN)                                                                                                     \
    hipLaunchKernelGGL((dsp::stft_kernel<NN>), grid, dim3(dsp::NT), 0, st, audio, L, d->hop, T, d->win, d->tw, d->W, \
                       d->lo, d->hi, d->n_mels, nullptr, static_cast<float2*>(out_spec))
    if (d->n_fft == 512) M2_STFT(512);
    else if (d->n_fft == 1024) M2_STFT(1024);
    else M2_STFT(2048);
#undef M2_STFT
    M2_LAUNCHED("stft_kernel");
    return M2_OK;
}

int32_t m2_mel_spectrogram(const m2_dsp* d, const float* audio, int32_t B, int32_t L, float* out_mel, void* stream) {
    M2_CHECK_ARG(d && B >= 0 && L > 0 && (B == 0 || (audio && out_mel)), "m2_mel_spectrogram: bad argument");
    if (B == 0) return M2_OK;
    const int T = frames_of(d, L);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(T, B);
#define M2_MEL(NN)                                                                                                      \
    hipLaunchKernelGGL((dsp::stft_kernel<NN>), grid, dim3(dsp::NT), 0, st, audio, L, d->hop, T, d->win, d->tw, d->W, \
                       d->lo, d->hi, d->n_mels, out_mel, nullptr)
    if (d->n_fft == 512) M2_MEL(512);
    else if (d->n_fft == 1024) M2_MEL(1024);
    else M2_MEL(2048);
#undef M2_MEL
    M2_LAUNCHED("stft_kernel(mel)");
    hipLaunchKernelGGL(dsp::db_norm_kernel, dim3(B), dim3(1024), 0, st, out_mel, d->n_mels * T);
    M2_LAUNCHED("db_norm_kernel");
    return M2_OK;
}

size_t m2_mel_features_ragged_workspace_bytes(const m2_dsp* d, int32_t B, int64_t total_samples) {
    if (!d || B < 0 || total_samples < 0) return 0;
    Sizer s;
    carve_ragged(s, d, B, total_samples, nullptr);
    return s.off + 256;
}

int32_t m2_mel_features_ragged(const m2_dsp* d, const void* samples, int32_t sample_format, const int64_t* offsets,
                               const int64_t* offsets_host, int32_t B, int32_t normalize, int32_t max_frames,
                               float* out_mel, int32_t T_out, int32_t* out_frames, void* workspace,
                               size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(d && B >= 0 && max_frames >= 0 && T_out >= 0 &&
                     (sample_format == M2_SAMPLES_F32 || sample_format == M2_SAMPLES_I16),
                 "m2_mel_features_ragged: bad argument");
    if (B == 0) return M2_OK;
    M2_CHECK_ARG(samples && offsets && offsets_host && out_frames && (out_mel || T_out == 0),
                 "m2_mel_features_ragged: bad argument");
    M2_CHECK_ARG(offsets_host[0] == 0, "m2_mel_features_ragged: offsets[0] must be 0");
    int64_t frames = 0, keep_max = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t L = offsets_host[b + 1] - offsets_host[b];
        M2_CHECK_SHAPE(L > 0, "m2_mel_features_ragged: an utterance has no samples");
        M2_CHECK_SHAPE(offsets_host[b + 1] < ((int64_t)1 << 31), "m2_mel_features_ragged: 2^31 samples or more in one call");
        const int64_t T = 1 + L / d->hop;
        frames += T;
        keep_max = std::max(keep_max, max_frames > 0 ? std::min<int64_t>(T, max_frames) : T);
    }
    const int64_t total = offsets_host[B];
    M2_CHECK_SHAPE((int64_t)d->n_mels * frames < ((int64_t)1 << 31),
                   "m2_mel_features_ragged: n_mels x frames reaches 2^31 in one call");
    M2_CHECK_SHAPE(T_out >= keep_max, "m2_mel_features_ragged: T_out is smaller than the largest stored frame count");
    Carve c(workspace, workspace_bytes);
    RaggedBufs w;
    carve_ragged(c, d, B, total, &w);
    if (!c.ok) return fail(M2_E_WORKSPACE, "m2_mel_features_ragged: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dsp::RaggedSamples smp{samples, sample_format};
    hipLaunchKernelGGL(dsp::ragged_prep_kernel, dim3(1), dim3(dsp::kPrepNT), 0, st, offsets, B, d->hop, max_frames, w.fp,
                       w.peak, out_frames);
    M2_LAUNCHED("ragged_prep_kernel");
    if (normalize) {
        hipLaunchKernelGGL(dsp::ragged_peak_kernel, dim3((unsigned)((total + dsp::kPeakChunk - 1) / dsp::kPeakChunk)),
                           dim3(dsp::NT), 0, st, smp, offsets, B, w.peak);
        M2_LAUNCHED("ragged_peak_kernel");
    }
#define M2_RFRAME(NN)                                                                                             \
    hipLaunchKernelGGL((dsp::ragged_frame_kernel<NN>), dim3((unsigned)frames), dim3(dsp::NT), 0, st, smp, offsets, \
                       w.fp, B, d->hop, normalize ? w.peak : nullptr, d->win, d->tw, d->W, d->lo, d->hi, d->n_mels, w.raw)
    if (d->n_fft == 512) M2_RFRAME(512);
    else if (d->n_fft == 1024) M2_RFRAME(1024);
    else M2_RFRAME(2048);
#undef M2_RFRAME
    M2_LAUNCHED("ragged_frame_kernel");
    hipLaunchKernelGGL(dsp::ragged_db_norm_kernel, dim3(B), dim3(1024), 0, st, w.raw, w.fp, d->n_mels, out_frames, T_out,
                       out_mel);
    M2_LAUNCHED("ragged_db_norm_kernel");
    return M2_OK;
}

size_t m2_mel_to_magnitude_workspace_bytes(const m2_dsp* d, int32_t B, int32_t T) {
    if (!d || B < 0 || T < 0) return 0;
    Sizer s;
    carve_nnls(s, B, T, nullptr);
    return s.off + 256;
}

int32_t m2_mel_to_magnitude(const m2_dsp* d, const float* mel, int32_t B, int32_t T, int32_t nnls_iters,
                            float* out_mag, void* workspace, size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(d && B >= 0 && T >= 0 && nnls_iters >= 0 && (B == 0 || T == 0 || (mel && out_mag)),
                 "m2_mel_to_magnitude: bad argument");
    if (B == 0 || T == 0) return M2_OK;
    Carve c(workspace, workspace_bytes);
    float* pg;
    carve_nnls(c, B, T, &pg);
    if (!c.ok) return fail(M2_E_WORKSPACE, "m2_mel_to_magnitude: workspace too small");
    return nnls_magnitudes(d, mel, B, T, nnls_iters, out_mag, pg, static_cast<hipStream_t>(stream));
}

size_t m2_griffin_lim_workspace_bytes(const m2_dsp* d, int32_t B, int32_t T) {
    if (!d || B < 0 || T < 0) return 0;
    Sizer s;
    carve_griffin_lim(s, d, B, T, nullptr);
    return s.off + 256;
}

// mag: if non-null the magnitudes [B, T, F] are taken from it (no mel / NNLS);
// else they come from mel [B, n_mels, T] (normalised dB, audio.py:128-132).
int32_t m2_griffin_lim(const m2_dsp* d, const float* mel, const float* mag, const void* init_angles, int32_t B,
                       int32_t T, int32_t n_iter, float momentum, int32_t nnls_iters, float* out_audio,
                       void* workspace, size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(d && B >= 0 && T >= 1 && n_iter >= 0 && nnls_iters >= 0, "m2_griffin_lim: bad argument");
    M2_CHECK_SHAPE(T >= 2, "m2_griffin_lim: need at least 2 frames");  // before the pointers: T = 1 has no output
    if (B == 0) return M2_OK;
    M2_CHECK_ARG((mel || mag) && init_angles && out_audio, "m2_griffin_lim: bad argument");
    const int N = d->n_fft, F = N / 2 + 1, Lout = d->hop * (T - 1);
    Carve c(workspace, workspace_bytes);
    GriffinLimBufs w;
    carve_griffin_lim(c, d, B, T, &w);
    if (!c.ok) return fail(M2_E_WORKSPACE, "m2_griffin_lim: workspace too small");
    float *S = w.S, *fr = w.fr, *y = w.y, *pgw = w.pg;
    float2 *ang = w.ang, *prev = w.prev;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 fgrid(T, B);
    if (mag) {
        M2_HIP(hipMemcpyAsync(S, mag, (size_t)B * T * F * sizeof(float), hipMemcpyDeviceToDevice, st));
    } else {
        int32_t rc;
        if ((rc = nnls_magnitudes(d, mel, B, T, nnls_iters, S, pgw, st))) return rc;
    }
    M2_HIP(hipMemcpyAsync(ang, init_angles, (size_t)B * T * F * sizeof(float2), hipMemcpyDeviceToDevice, st));
    M2_HIP(hipMemsetAsync(prev, 0, (size_t)B * T * F * sizeof(float2), st));
    const dim3 ogrid(cdiv(Lout, 256), B);
    auto istft = [&](float* dst) -> int32_t {
#define M2_ISTFT(NN)                                                                                              \
    do {                                                                                                          \
        hipLaunchKernelGGL((dsp::istft_frame_kernel<NN>), fgrid, dim3(dsp::NT), 0, st, S, ang, T, d->win, d->tw, fr); \
        hipLaunchKernelGGL((dsp::ola_kernel<NN>), ogrid, dim3(256), 0, st, fr, T, d->hop, d->win, Lout, dst);       \
    } while (0)
        if (N == 512) M2_ISTFT(512);
        else if (N == 1024) M2_ISTFT(1024);
        else M2_ISTFT(2048);
#undef M2_ISTFT
        M2_LAUNCHED("istft");
        return M2_OK;
    };
    for (int it = 0; it < n_iter; ++it) {
        int32_t rc = istft(y);
        if (rc) return rc;
#define M2_GLU(NN)                                                                                                   \
    hipLaunchKernelGGL((dsp::gl_update_kernel<NN>), fgrid, dim3(dsp::NT), 0, st, y, Lout, d->hop, T, d->win, d->tw, \
                       momentum, ang, prev)
        if (N == 512) M2_GLU(512);
        else if (N == 1024) M2_GLU(1024);
        else M2_GLU(2048);
#undef M2_GLU
        M2_LAUNCHED("gl_update_kernel");
    }
    int32_t rc = istft(out_audio);
    if (rc) return rc;
    if (mel) {  // mel_to_audio's peak normalisation (audio.py:146-147); not for the bare Griffin-Lim
        hipLaunchKernelGGL(dsp::peak_norm_kernel, dim3(B), dim3(1024), 0, st, out_audio, Lout);
        M2_LAUNCHED("peak_norm_kernel");
    }
    return M2_OK;
}

}  // extern "C"
