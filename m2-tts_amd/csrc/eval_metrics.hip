// Evaluation metrics on the GPU: the sums behind the reference's
// src/evaluation/metrics.py (estimate_mos_score, compute_mel_distance,
// compute_duration_accuracy, compute_mcd), batched over utterances.  The
// kernels produce per-utterance rows of double sums; the scalar finishing
// (logs, clips, weights) is the caller's, on the host.
//
//   audio   eval_frame_kernel: one workgroup per (frame, utterance).  With a
//           target the two real frames share one complex FFT,
//           z = pred win + i target win, and are separated by the Hermitian
//           symmetry: P[f] = (Z[f] + conj Z[N-f]) / 2,
//           T[f] = (Z[f] - conj Z[N-f]) / 2i.  Both signals are cut to
//           L = min(Lp, Lt) first (metrics.py:95-97).  The centroid and the
//           bandwidth belong to the un-cut pred (metrics.py:119): a frame
//           whose window reaches past L while the pred goes on takes them
//           from a second, plain FFT of the pred alone.  No spectrum leaves
//           LDS; a frame stores five doubles.
//           eval_time_kernel: the time-domain sums per 4096-sample chunk.
//           eval_finish_kernel: one workgroup per utterance adds the frame
//           and chunk partials in a fixed order, in double.
//   pairs   pair_stats_kernel: one workgroup per utterance over [R, C]
//           (pred optionally stored [C, R]), two passes (means, then the
//           centred second moments, so a constant row has variance exactly 0).
//   mcd     mcd_kernel: one thread per frame, 13 DCT-II rows against
//           pred - target (the DCT is linear), in double.
// Every reduction is a lane-strided sum, an xor-shuffle tree and the wave
// partials in order: no floating-point atomics, so two runs give equal bits.
#include <cfloat>
#include <cmath>

#include "audio_dsp.h"

namespace m2 {
namespace eval {

using dsp::block_sum;
using dsp::NT;

constexpr int kFramePart = 5;   // per frame: err^2, ref^2, log^2, centroid, bandwidth
constexpr int kChunkPart = 4;   // per chunk: target^2, noise^2, pred^2, sign changes
constexpr int kChunk = 4096;    // samples per eval_time_kernel workgroup
constexpr int kMcdCoef = 13;    // librosa.feature.mfcc(n_mfcc=13), metrics.py:64-65

const char* const kAudioCols[] = {"spec_err_sq", "spec_ref_sq", "log_spec_sq", "pair_bins",    "target_sq",
                                  "noise_sq",    "pair_len",    "pred_sq",     "sign_changes", "pred_len",
                                  "centroid_sum", "bandwidth_sum", "pred_frames"};
const char* const kPairCols[] = {"abs_diff", "sq_diff", "sum_p", "sum_t", "sum_pp", "sum_tt",
                                 "sum_pt",   "count",   "cen_pp", "cen_tt", "cen_pt"};
const char* const kMcdCols[] = {"mcd_sum", "frames"};
constexpr int kAudioK = sizeof(kAudioCols) / sizeof(kAudioCols[0]);
constexpr int kPairK = sizeof(kPairCols) / sizeof(kPairCols[0]);
constexpr int kMcdK = sizeof(kMcdCols) / sizeof(kMcdCols[0]);

// grid (frames of the un-cut pred, B); part [B, frames, kFramePart].
template <int N>
__global__ __launch_bounds__(NT) void eval_frame_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                        int Lp, int Lt, int L, int hop, int frames_pair, int sr,
                                                        const float* __restrict__ win, const float2* __restrict__ tw,
                                                        double* __restrict__ part) {
    __shared__ float2 a[N], b[N];
    __shared__ float mag[N / 2 + 1];
    __shared__ double red[NT / 64];
    constexpr int F = N / 2 + 1;
    const int t = blockIdx.x, u = blockIdx.y, frames = gridDim.x;
    const float* p = pred + (size_t)u * Lp;
    const bool paired = target != nullptr && t < frames_pair;
    // the cut changes the pred frame only where the window reaches past L and the pred goes on
    const bool own = !paired || (Lp > L && t * hop + N / 2 > L);
    double err = 0.0, ref = 0.0, lsd = 0.0;
    if (paired) {
        dsp::load_pair_frame<N>(p, target + (size_t)u * Lt, L, hop, t, win, a);
        const float2* Z = dsp::fft_lds<N, false>(a, b, tw);
        for (int f = threadIdx.x; f < F; f += NT) {
            const float2 zf = Z[f], zn = Z[(N - f) & (N - 1)];
            const float pr = 0.5f * (zf.x + zn.x), pi = 0.5f * (zf.y - zn.y);
            const float tr = 0.5f * (zf.y + zn.y), ti = 0.5f * (zn.x - zf.x);
            const float mp = sqrtf(pr * pr + pi * pi), mt = sqrtf(tr * tr + ti * ti);
            if (!own) mag[f] = mp;
            const double d = (double)mt - (double)mp;
            err += d * d;
            ref += (double)mt * (double)mt;
            const double l = log((double)mp + 1e-8) - log((double)mt + 1e-8);
            lsd += l * l;
        }
        err = block_sum(err, red);
        ref = block_sum(ref, red);
        lsd = block_sum(lsd, red);
    }
    if (own) {  // block_sum's barriers are behind every read of Z
        dsp::load_frame<N>(p, Lp, hop, t, win, a);
        const float2* X = dsp::fft_lds<N, false>(a, b, tw);
        for (int f = threadIdx.x; f < F; f += NT) mag[f] = sqrtf(X[f].x * X[f].x + X[f].y * X[f].y);
    }
    __syncthreads();
    const double hz = (double)sr / (double)N;
    double s0 = 0.0, s1 = 0.0;
    for (int f = threadIdx.x; f < F; f += NT) {
        s0 += (double)mag[f];
        s1 += (double)f * hz * (double)mag[f];
    }
    s0 = block_sum(s0, red);
    s1 = block_sum(s1, red);
    const double norm = s0 < (double)FLT_MIN ? 1.0 : s0;  // librosa.util.normalize(norm=1)
    const double cen = s1 / norm;
    double s2 = 0.0;
    for (int f = threadIdx.x; f < F; f += NT) {
        const double dev = (double)f * hz - cen;
        s2 += (double)mag[f] / norm * dev * dev;
    }
    s2 = block_sum(s2, red);
    if (threadIdx.x == 0) {
        double* o = part + ((size_t)u * frames + t) * kFramePart;
        o[0] = err;
        o[1] = ref;
        o[2] = lsd;
        o[3] = cen;
        o[4] = sqrt(s2);
    }
}

__device__ __forceinline__ float sign_of(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

// grid (chunks of the un-cut pred, B); part [B, chunks, kChunkPart].
__global__ __launch_bounds__(NT) void eval_time_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                       int Lp, int Lt, int L, double* __restrict__ part) {
    __shared__ double red[NT / 64];
    const int c = blockIdx.x, u = blockIdx.y, chunks = gridDim.x;
    const float* p = pred + (size_t)u * Lp;
    const float* q = target ? target + (size_t)u * Lt : nullptr;
    const long long i0 = (long long)c * kChunk;
    const long long i1 = i0 + kChunk < (long long)Lp ? i0 + kChunk : (long long)Lp;
    double tt = 0.0, nn = 0.0, pp = 0.0, zc = 0.0;
    for (long long i = i0 + threadIdx.x; i < i1; i += NT) {
        const float x = p[i];
        pp += (double)x * (double)x;
        if (i + 1 < Lp) zc += (double)fabsf(sign_of(p[i + 1]) - sign_of(x));
        if (q && i < L) {
            const double r = (double)q[i], d = (double)x - r;
            tt += r * r;
            nn += d * d;
        }
    }
    tt = block_sum(tt, red);
    nn = block_sum(nn, red);
    pp = block_sum(pp, red);
    zc = block_sum(zc, red);
    if (threadIdx.x == 0) {
        double* o = part + ((size_t)u * chunks + c) * kChunkPart;
        o[0] = tt;
        o[1] = nn;
        o[2] = pp;
        o[3] = zc;
    }
}

// grid (B): out [B, kAudioK] from the partials, added in a fixed order.
__global__ __launch_bounds__(NT) void eval_finish_kernel(const double* __restrict__ fpart, int frames,
                                                         const double* __restrict__ cpart, int chunks,
                                                         int frames_pair, int F, int Lp, int L,
                                                         double* __restrict__ out) {
    __shared__ double red[NT / 64];
    const int u = blockIdx.x;
    const double* fp = fpart + (size_t)u * frames * kFramePart;
    const double* cp = cpart + (size_t)u * chunks * kChunkPart;
    double fs[kFramePart], cs[kChunkPart];
    for (int k = 0; k < kFramePart; ++k) {
        double s = 0.0;
        for (int i = threadIdx.x; i < frames; i += NT) s += fp[(size_t)i * kFramePart + k];
        fs[k] = block_sum(s, red);
    }
    for (int k = 0; k < kChunkPart; ++k) {
        double s = 0.0;
        for (int i = threadIdx.x; i < chunks; i += NT) s += cp[(size_t)i * kChunkPart + k];
        cs[k] = block_sum(s, red);
    }
    if (threadIdx.x == 0) {
        double* o = out + (size_t)u * kAudioK;
        o[0] = fs[0];
        o[1] = fs[1];
        o[2] = fs[2];
        o[3] = (double)frames_pair * (double)F;
        o[4] = cs[0];
        o[5] = cs[1];
        o[6] = (double)L;
        o[7] = cs[2];
        o[8] = cs[3];
        o[9] = (double)Lp;
        o[10] = fs[3];
        o[11] = fs[4];
        o[12] = (double)frames;
    }
}

// grid (B): target [B, R, C]; pred [B, R, C], or [B, C, R] when transposed;
// cols[b] (optional) keeps the first min(cols[b], C) columns; out [B, kPairK].
__global__ __launch_bounds__(NT) void pair_stats_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                        const int32_t* __restrict__ cols, int R, int C, int transposed,
                                                        double* __restrict__ out) {
    __shared__ double red[NT / 64];
    const int u = blockIdx.x;
    const float* p = pred + (size_t)u * R * C;
    const float* q = target + (size_t)u * R * C;
    int c = C;
    if (cols) c = min(C, max(0, cols[u]));
    const long long n = (long long)R * c;
    double s[7] = {0, 0, 0, 0, 0, 0, 0};
    for (long long i = threadIdx.x; i < n; i += NT) {
        const int r = (int)(i / c), k = (int)(i % c);
        const double b = (double)q[(size_t)r * C + k];
        const double a = (double)(transposed ? p[(size_t)k * R + r] : p[(size_t)r * C + k]);
        const double d = a - b;
        s[0] += fabs(d);
        s[1] += d * d;
        s[2] += a;
        s[3] += b;
        s[4] += a * a;
        s[5] += b * b;
        s[6] += a * b;
    }
    for (int k = 0; k < 7; ++k) s[k] = block_sum(s[k], red);
    const double ma = n > 0 ? s[2] / (double)n : 0.0, mb = n > 0 ? s[3] / (double)n : 0.0;
    double m[3] = {0, 0, 0};
    for (long long i = threadIdx.x; i < n; i += NT) {
        const int r = (int)(i / c), k = (int)(i % c);
        const double b = (double)q[(size_t)r * C + k] - mb;
        const double a = (double)(transposed ? p[(size_t)k * R + r] : p[(size_t)r * C + k]) - ma;
        m[0] += a * a;
        m[1] += b * b;
        m[2] += a * b;
    }
    for (int k = 0; k < 3; ++k) m[k] = block_sum(m[k], red);
    if (threadIdx.x == 0) {
        double* o = out + (size_t)u * kPairK;
        for (int k = 0; k < 7; ++k) o[k] = s[k];
        o[7] = (double)n;
        for (int k = 0; k < 3; ++k) o[8 + k] = m[k];
    }
}

// grid (B): target [B, M, Tt]; pred [B, M, Tp], or [B, Tp, M] when
// transposed; frames = min(Tp, Tt, cols[b]); table [kMcdCoef, M] doubles;
// out [B, kMcdK] = sum over frames of sqrt(sum_c (table (pred - target))_c^2), frames.
__global__ __launch_bounds__(NT) void mcd_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                 const int32_t* __restrict__ cols, const double* __restrict__ table,
                                                 int M, int Tp, int Tt, int transposed, double* __restrict__ out) {
    __shared__ double red[NT / 64];
    const int u = blockIdx.x;
    const float* p = pred + (size_t)u * M * Tp;
    const float* q = target + (size_t)u * M * Tt;
    int n = min(Tp, Tt);
    if (cols) n = min(n, max(0, cols[u]));
    double s = 0.0;
    for (int t = threadIdx.x; t < n; t += NT) {
        double acc[kMcdCoef];
        for (int c = 0; c < kMcdCoef; ++c) acc[c] = 0.0;
        for (int m = 0; m < M; ++m) {
            const float a = transposed ? p[(size_t)t * M + m] : p[(size_t)m * Tp + t];
            const double d = (double)a - (double)q[(size_t)m * Tt + t];
#pragma unroll
            for (int c = 0; c < kMcdCoef; ++c) acc[c] += table[(size_t)c * M + m] * d;
        }
        double e = 0.0;
        for (int c = 0; c < kMcdCoef; ++c) e += acc[c] * acc[c];
        s += sqrt(e);
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
        out[(size_t)u * kMcdK] = s;
        out[(size_t)u * kMcdK + 1] = (double)n;
    }
}

}  // namespace eval
}  // namespace m2

namespace {
using namespace m2;

constexpr int kMaxGridY = 65535;

int chunks_of(int Lp) { return cdiv(Lp, eval::kChunk); }

// m2_eval_audio's workspace, written once: the partials of eval_frame_kernel [B, frames, kFramePart]
// and of eval_time_kernel [B, chunks, kChunkPart].
template <typename A>
void carve_eval_audio(A& a, const m2_dsp* d, int B, int Lp, double** fpart, double** cpart) {
    double* f = a.template take<double>((size_t)B * (1 + Lp / d->hop) * eval::kFramePart);
    double* c = a.template take<double>((size_t)B * chunks_of(Lp) * eval::kChunkPart);
    if (fpart) *fpart = f, *cpart = c;
}
}  // namespace

extern "C" {

int32_t m2_eval_column_count(int32_t kind) {
    return kind == 0 ? eval::kAudioK : kind == 1 ? eval::kPairK : kind == 2 ? eval::kMcdK : -1;
}

const char* m2_eval_column_name(int32_t kind, int32_t index) {
    if (index < 0 || index >= m2_eval_column_count(kind)) return nullptr;
    return kind == 0 ? eval::kAudioCols[index] : kind == 1 ? eval::kPairCols[index] : eval::kMcdCols[index];
}

size_t m2_eval_audio_workspace_bytes(const m2_dsp* d, int32_t B, int32_t Lp) {
    if (!d || B < 0 || Lp < 0) return 0;
    Sizer s;
    carve_eval_audio(s, d, B, Lp, nullptr, nullptr);
    return s.off + 256;
}

int32_t m2_eval_audio(const m2_dsp* d, const float* pred, const float* target, int32_t B, int32_t Lp, int32_t Lt,
                      double* out, void* workspace, size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(d && pred && out && B >= 0 && Lp > 0 && (!target || Lt > 0), "m2_eval_audio: bad argument");
    M2_CHECK_SHAPE(B <= kMaxGridY && Lp <= (1 << 30), "m2_eval_audio: at most 65535 utterances of at most 2^30 samples");
    if (B == 0) return M2_OK;
    const int L = target ? (Lp < Lt ? Lp : Lt) : 0;
    const int frames = 1 + Lp / d->hop, frames_pair = target ? 1 + L / d->hop : 0, chunks = chunks_of(Lp);
    if (!target) Lt = 0;
    Carve c(workspace, workspace_bytes);
    double *fpart, *cpart;
    carve_eval_audio(c, d, B, Lp, &fpart, &cpart);
    if (!c.ok) return fail(M2_E_WORKSPACE, "m2_eval_audio: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
#define M2_EVAL(NN)                                                                                                   \
    hipLaunchKernelGGL((eval::eval_frame_kernel<NN>), dim3(frames, B), dim3(dsp::NT), 0, st, pred, target, Lp, Lt, L, \
                       d->hop, frames_pair, d->sr, d->win, d->tw, fpart)
    if (d->n_fft == 512) M2_EVAL(512);
    else if (d->n_fft == 1024) M2_EVAL(1024);
    else M2_EVAL(2048);
#undef M2_EVAL
    M2_LAUNCHED("eval_frame_kernel");
    hipLaunchKernelGGL(eval::eval_time_kernel, dim3(chunks, B), dim3(dsp::NT), 0, st, pred, target, Lp, Lt, L, cpart);
    M2_LAUNCHED("eval_time_kernel");
    hipLaunchKernelGGL(eval::eval_finish_kernel, dim3(B), dim3(dsp::NT), 0, st, fpart, frames, cpart, chunks,
                       frames_pair, d->n_fft / 2 + 1, Lp, L, out);
    M2_LAUNCHED("eval_finish_kernel");
    return M2_OK;
}

int32_t m2_eval_pair_stats(const float* pred, const float* target, const int32_t* cols, int32_t B, int32_t R,
                           int32_t C, int32_t pred_transposed, double* out, void* stream) {
    M2_CHECK_ARG(pred && target && out && B >= 0 && R > 0 && C > 0, "m2_eval_pair_stats: bad argument");
    if (B == 0) return M2_OK;
    hipLaunchKernelGGL(eval::pair_stats_kernel, dim3(B), dim3(dsp::NT), 0, static_cast<hipStream_t>(stream), pred,
                       target, cols, R, C, pred_transposed != 0, out);
    M2_LAUNCHED("pair_stats_kernel");
    return M2_OK;
}

int32_t m2_eval_mcd_coefficients(void) { return eval::kMcdCoef; }

int32_t m2_eval_dct_table(int32_t n_mels, double* out_host) {
    M2_CHECK_ARG(out_host && n_mels > 0, "m2_eval_dct_table: bad argument");
    // scipy.fftpack.dct(type=2, norm='ortho') rows 0 .. 12; a transform of fewer
    // than 13 bands has no further rows (zeros here)
    for (int k = 0; k < eval::kMcdCoef; ++k) {
        const double sc = k < n_mels ? std::sqrt((k == 0 ? 1.0 : 2.0) / n_mels) : 0.0;
        for (int m = 0; m < n_mels; ++m)
            out_host[(size_t)k * n_mels + m] = sc * std::cos(M_PI * k * (2.0 * m + 1.0) / (2.0 * n_mels));
    }
    return M2_OK;
}

int32_t m2_eval_mcd(const float* pred, const float* target, const int32_t* cols, const double* table, int32_t B,
                    int32_t n_mels, int32_t Tp, int32_t Tt, int32_t pred_transposed, double* out, void* stream) {
    M2_CHECK_ARG(pred && target && table && out && B >= 0 && n_mels > 0 && Tp > 0 && Tt > 0,
                 "m2_eval_mcd: bad argument");
    if (B == 0) return M2_OK;
    hipLaunchKernelGGL(eval::mcd_kernel, dim3(B), dim3(dsp::NT), 0, static_cast<hipStream_t>(stream), pred, target,
                       cols, table, n_mels, Tp, Tt, pred_transposed != 0, out);
    M2_LAUNCHED("mcd_kernel");
    return M2_OK;
}

}  // extern "C"
