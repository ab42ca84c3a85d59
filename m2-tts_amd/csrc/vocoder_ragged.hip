// Ragged batches (m2_vocoder_ragged, m2_inference_back_ragged): the end of
// each utterance of a batch vocoded at the batch's longest frame count T.
//
// The batched vocoder call gives utterance b (T_b = frames[b] < T frames) the
// samples it would have alone for every frame whose receptive field (kRedoHalo
// mel frames per side) stays inside the utterance: frames < T_b - kRedoHalo.
// The last kRedoHalo frames saw the rows past T_b where the single call has
// the reference's zero padding.  They are computed again at the utterance's
// own length:
//  - T_b >= 2 kRedoHalo: the mel rows [T_b - 2 kRedoHalo, T_b) of every such
//    utterance are gathered into one [B, 2 kRedoHalo] batch (ragged_gather),
//    the caller runs the model's own vocoder kernels on it - its right edge is
//    the utterance's end, its left halo keeps the left edge out of the centre,
//    as in the streamed vocoder's windows - and the last kRedoHalo frames of
//    that audio replace the utterance's (ragged_scatter);
//  - shorter utterances (the window would be the whole utterance, each of its
//    own length): ragged_tail_kernel recomputes them in fp32 by direct
//    convolution with redo_frames (vocoder_redo.h), one workgroup per
//    utterance.  1.4 ms at stage2 widths, 0.39 ms at stage1 (MI355X, measured
//    when it still served every utterance): a path for degenerate utterances
//    only.
// ragged_zero_kernel clears what lies past each utterance's end.  None of this
// depends on which kernels the main pass ran (split-f16, exact-f32, streamed).
#include <algorithm>
#include <cstdint>

#include "m2_common.h"
#include "vocoder_redo.h"

namespace m2 {

namespace {
constexpr int kRaggedThreads = 1024;
// frames of the end window: kRedoHalo output frames and their left halo
constexpr int kRaggedWin = 2 * kRedoHalo;

// ragged_tail_kernel's LDS: the redo's buffers and, for [B][M][T] mels, the
// utterance's (< kRaggedWin) rows
__host__ __device__ constexpr int ragged_lds_floats(int M, int C) {
    return redo_lds_floats(C, kRedoHalo) + kRaggedWin * M;
}

// Frame count of utterance b as the ragged entry points read it.
__device__ __forceinline__ int ragged_frames(const int32_t* __restrict__ frames, int b, int T) {
    return min(max(frames[b], 1), T);
}

// Which pass redoes the end of a T_b-frame utterance of a T-frame batch: none
// when T_b == T (its end is the batch's), the window pass, or the fp32 kernel.
__device__ __forceinline__ bool ragged_window(int Tb, int T) { return Tb < T && Tb >= kRaggedWin; }
__device__ __forceinline__ bool ragged_direct(int Tb, int T) { return Tb < T && Tb < kRaggedWin; }

// wmel [B][kRaggedWin][M] (trans) or [B][M][kRaggedWin] := the last kRaggedWin
// rows of each window-pass utterance, zeros for the others.
__global__ __launch_bounds__(256) void ragged_gather_kernel(const float* __restrict__ mel, int trans,
                                                           const int32_t* __restrict__ frames, int T, int M,
                                                           float* __restrict__ wmel) {
    const int b = blockIdx.x, Tb = ragged_frames(frames, b, T), r0 = Tb - kRaggedWin;
    const bool live = ragged_window(Tb, T);
    float* w = wmel + (size_t)b * kRaggedWin * M;
    const float* mb = mel + (size_t)b * M * T;
    for (int idx = threadIdx.x; idx < kRaggedWin * M; idx += blockDim.x) {
        float v = 0.f;
        if (live) {
            if (trans) {
                v = mb[(size_t)r0 * M + idx];  // rows are contiguous
            } else {
                const int c = idx / kRaggedWin, r = idx - c * kRaggedWin;
                v = mb[(size_t)c * T + r0 + r];
            }
        }
        w[idx] = v;
    }
}

// audio[b][64 (T_b - kRedoHalo), 64 T_b) := the last kRedoHalo frames of the
// window pass's audio waudio [B][64 kRaggedWin].
__global__ __launch_bounds__(64 * kRedoHalo) void ragged_scatter_kernel(const float* __restrict__ waudio,
                                                                       const int32_t* __restrict__ frames, int T,
                                                                       float* __restrict__ audio) {
    const int b = blockIdx.x, Tb = ragged_frames(frames, b, T);
    if (!ragged_window(Tb, T)) return;
    audio[(size_t)b * 64 * T + 64 * (size_t)(Tb - kRedoHalo) + threadIdx.x] =
        waudio[(size_t)b * 64 * kRaggedWin + 64 * (kRaggedWin - kRedoHalo) + threadIdx.x];
}

// audio [B][64 T]; mel [B][T][M] (trans) or [B][M][T]: the utterances shorter
// than the end window, whole, in fp32.
__global__ __launch_bounds__(kRaggedThreads) void ragged_tail_kernel(const VocRedoW* __restrict__ rw,
                                                                    const float* __restrict__ mel, int trans,
                                                                    const int32_t* __restrict__ frames, int T,
                                                                    float* __restrict__ audio) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x, Tb = ragged_frames(frames, b, T);
    if (!ragged_direct(Tb, T)) return;  // workgroup-uniform
    const int M = rw->M, C = rw->C, nredo = redo_lds_floats(C, kRedoHalo);
    const int f0 = max(0, Tb - kRedoHalo);
    float* arow = audio + (size_t)b * 64 * T;
    if (trans) {  // the utterance's own rows, zero padding at T_b
        redo_frames(*rw, mel + (size_t)b * T * M, true, Tb, 0, f0, Tb, arow, lds, nredo);
        return;
    }
    // [B][M][T]: the rows of a T_b-frame utterance do not sit at pitch T_b, so
    // they are gathered as [row][M] into LDS first
    float* g = lds + nredo;
    const float* mb = mel + (size_t)b * M * T;
    for (int idx = threadIdx.x; idx < Tb * M; idx += blockDim.x) {
        const int c = idx / Tb, r = idx - c * Tb;
        g[r * M + c] = mb[(size_t)c * T + r];
    }
    __syncthreads();
    redo_frames(*rw, g, true, Tb, 0, f0, Tb, arow, lds, nredo);
}

// Rows [T_b, T) of x [B][T][W] := 0 (vector stores; V4: 16-B aligned rows).
template <bool V4>
__global__ __launch_bounds__(256) void ragged_zero_kernel(float* __restrict__ x, const int32_t* __restrict__ frames,
                                                         int T, int W) {
    const int b = blockIdx.y, Tb = ragged_frames(frames, b, T);
    const size_t n = (size_t)(T - Tb) * W, step = (size_t)gridDim.x * blockDim.x;
    float* p = x + ((size_t)b * T + Tb) * W;
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (V4) {
        float4* p4 = reinterpret_cast<float4*>(p);
        for (size_t i = i0; i < n / 4; i += step) p4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        for (size_t i = i0; i < n; i += step) p[i] = 0.f;
    }
}

// out[b] = max(1, tot[b]): the reference's frame count of utterance b alone
// (an utterance with no frames is one zero frame, tts_model.py:158-160).
__global__ void ragged_count_kernel(const int32_t* __restrict__ tot, int B, int32_t* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) out[b] = max(1, tot[b]);
}
}  // namespace

int32_t launch_ragged_count(const int32_t* tot, int B, int32_t* out, hipStream_t st) {
    if (B == 0) return M2_OK;
    hipLaunchKernelGGL(ragged_count_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, tot, B, out);
    M2_LAUNCHED("ragged_count_kernel");
    return M2_OK;
}

int32_t launch_ragged_zero(float* x, const int32_t* frames, int B, int T, int W, hipStream_t st) {
    if (B == 0 || T == 0 || W == 0) return M2_OK;
    const bool v4 = W % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0;
    // enough workgroups for a whole row set of one utterance, capped: the
    // kernel strides over what is left
    const size_t per = (size_t)T * W / (v4 ? 4 : 1);
    const dim3 grid((unsigned)std::min<size_t>(std::max<size_t>(1, (per + 255) / 256), 64), B);
    if (v4) hipLaunchKernelGGL(ragged_zero_kernel<true>, grid, dim3(256), 0, st, x, frames, T, W);
    else hipLaunchKernelGGL(ragged_zero_kernel<false>, grid, dim3(256), 0, st, x, frames, T, W);
    M2_LAUNCHED("ragged_zero_kernel");
    return M2_OK;
}

int ragged_window_frames() { return kRaggedWin; }

int32_t launch_ragged_gather(const float* mel, bool trans, const int32_t* frames, int B, int T, int M, float* wmel,
                             hipStream_t st) {
    if (B == 0) return M2_OK;
    hipLaunchKernelGGL(ragged_gather_kernel, dim3(B), dim3(256), 0, st, mel, trans ? 1 : 0, frames, T, M, wmel);
    M2_LAUNCHED("ragged_gather_kernel");
    return M2_OK;
}

int32_t launch_ragged_scatter(const float* waudio, const int32_t* frames, int B, int T, float* audio, hipStream_t st) {
    if (B == 0) return M2_OK;
    hipLaunchKernelGGL(ragged_scatter_kernel, dim3(B), dim3(64 * kRedoHalo), 0, st, waudio, frames, T, audio);
    M2_LAUNCHED("ragged_scatter_kernel");
    return M2_OK;
}

// rw: the model's device copy of the fp32 vocoder weights (M mel channels, C
// vocoder channels: they size the dynamic LDS).
int32_t launch_ragged_tail(const VocRedoW* rw, int M, int C, const float* mel, bool trans, const int32_t* frames, int B,
                           int T, float* audio, hipStream_t st) {
    if (B == 0 || T == 0) return M2_OK;
    const int lds_bytes = ragged_lds_floats(M, C) * (int)sizeof(float);
    static int attr_bytes = 0;
    if (attr_bytes < lds_bytes) {
        M2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ragged_tail_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
        attr_bytes = lds_bytes;
    }
    hipLaunchKernelGGL(ragged_tail_kernel, dim3(B), dim3(kRaggedThreads), lds_bytes, st, rw, mel, trans ? 1 : 0, frames,
                       T, audio);
    M2_LAUNCHED("ragged_tail_kernel");
    return M2_OK;
}

}  // namespace m2
