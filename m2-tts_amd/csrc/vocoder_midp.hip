// Pipelined SimpleVocoder mid stage for stage1 (tts_model.py:279-297, the
// second upsampling stage): ConvT2 (64 -> 32 channels, x4, k 8, pad 2) +
// leaky, ResBlock2 (conv1 + leaky, conv2 + residual), split-f16 arithmetic
// (vocoder_x3.hip).  Reads U1 (the head kernel's output, rows of hi[64] lo[64]
// per position at 4T) and writes U2 (rows of hi[32] lo[32] at 16T), the
// formats of the x3 mid kernel it replaces.
//
// Polyphase form over the columns q of U1: ConvT2's output u2 (32 channels at
// t2 = 4q + s) is a 128-row column (phase s, channel) = 8 m-blocks of 16
// rows, m-block 2s + h holding channels 16h .. 16h+15 of phase s.
//   ConvT2, phase s:  s < 2: x[q] W[s+2] + x[q-1] W[s+6]
//                     s > 1: x[q+1] W[s-2] + x[q] W[s+2]
//     -> K = 2 taps x 64 channels = 4 k-blocks (tap, octet half).
//   ResBlock2 convs, phase s: taps t2-1, t2, t2+1 = phase (s+d) mod 4 of
//     column q + floor((s+d)/4), d = -1, 0, 1 -> K = 3 k-blocks, one whole
//     32-channel phase each: no padding.
// The two m-blocks of one phase read the same K slots, so one wave owns a
// phase (both m-blocks) and every B fragment it reads feeds two MFMA tiles.
//
// Systolic pipeline, one workgroup per CU (88 KB of LDS rings): a loader wave
// streams U1 into ring R0, 4 waves (one per phase) per layer compute 16
// columns per step each, one s_barrier per step, weights (8 / 6 fragment pairs
// per wave) in VGPRs for the whole strip - the structure of vocoder_tailp.hip
// (ring protocol, warm-up chunk -1, zero columns outside [0, L1), permlane16
// swapped 16-B epilogue stores).  The conv2 waves add the residual (ring R1,
// ConvT2's output) in the epilogue and store U2 rows straight to global.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "m2_common.h"
#include "vocoder_fused.h"
#include "vocoder_midp.h"  // the ring constants and layer_role
#include "vocoder_pipe.h"

namespace m2 {
namespace mp {

constexpr int R0_OFF = RingLay::R0_OFF, LDS_BYTES = RingLay::LDS_BYTES;
constexpr int NWAVES = 13;              // 4 phases x 3 layers + 1 loader (wave 12)

// U1 rows (256 B) into ring R0, two chunks ahead: chunk c = columns
// [qa + 3 + 16c, +16), zero outside [0, L1).  Four 16-B pieces per lane per
// chunk, loads issued unconditionally (clamped) so their waits are counted.
template <bool EDGE>
__device__ __forceinline__ void loader_role(unsigned char* lds, int qa, int L1, int nch,
                                            const unsigned char* __restrict__ u1) {
    const int lane = threadIdx.x & 63, cr = lane >> 4, pc = lane & 15;
    auto fetch = [&](int c, u32x4 (&v)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int col = qa + 3 + 16 * c + 4 * j + cr;
            if (EDGE) col = min(max(col, 0), L1 - 1);
            v[j] = *reinterpret_cast<const u32x4*>(u1 + (size_t)col * 256 + pc * 16);
        }
    };
    u32x4 buf[3][4];
    auto step = [&](int s, u32x4 (&cur)[4], u32x4 (&ahead)[4]) {
        fetch(min(s + 2, nch - 1), ahead);
        if (s < nch) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = qa + 3 + 16 * s + 4 * j + cr;
                const bool in = !EDGE || (col >= 0 && col < L1);
                const u32x4 z{0u, 0u, 0u, 0u};
                *reinterpret_cast<u32x4*>(lds + R0_OFF + ((16 * s + 4 * j + cr) & (RROWS - 1)) * RS0 + pc * 16) =
                    in ? cur[j] : z;
            }
        }
        step_barrier();
    };
    fetch(-1, buf[0]);
    fetch(0, buf[1]);
    int s = -1;
#pragma unroll 1
    for (; s + 2 <= nch + 2; s += 3) {
        step(s, buf[0], buf[2]);
        step(s + 1, buf[1], buf[0]);
        step(s + 2, buf[2], buf[1]);
    }
#pragma unroll 1
    for (; s <= nch + 2; ++s) step_barrier();
}

// MIDP_DMA (default): U1 rows into ring R0 by LDS-DMA (as the tails'
// loader_role_dma): a chunk's 16 ring rows are 16 x RS0 = 4,608 contiguous
// bytes (hi[64] lo[64] + 32 B of padding per row), written by five
// buffer_load_dwordx4 ... lds of 64 lanes x 16 B (the fifth by lanes 0-31
// only: EXEC-masked lanes write nothing, so the next chunk's rows are left
// alone).  Lane l of instruction i fills 16-B unit u = 64 i + l of the
// chunk: row u / 18, unit u % 18 of the row - units 0-15 are the U1 row's
// 16-B pieces in order, 16-17 the padding (loaded out of range: zeros).
// Columns outside [0, L1) are out of the descriptor's range and land as
// zeros.  Chunk c + 1 is issued at the top of step c into the slot of chunk
// c - 3; chunk c has landed before step c's barrier (vmcnt(5)).
// Measured level, so not the default (MIDP_DMA=1 builds it): midp 19.74 /
// 20.14 us against 19.83 / 19.86 us with the register loader, alternated on
// one box, 169 tests green on it (profiles/r06/r06u_mid_dma_ab/,
// r06u_tests.log) - the mid's loader is not on its step's critical path.
#ifndef MIDP_DMA
#define MIDP_DMA 0
#endif
__device__ __forceinline__ void loader_role_dma(unsigned char* lds, int qa, int L1, int nch,
                                                const unsigned char* __restrict__ u1) {
    static_assert(RROWS == 64 && RS0 == 288, "4-chunk R0 of 288-B rows");
    const int lane = threadIdx.x & 63;
    // descriptor from the strip's first column to the utterance's end
    const int c0 = max(0, qa + 3 - 16);
    [[maybe_unused]] const auto rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned char*>(u1) + (size_t)c0 * 256, 0, (int)min((long)(L1 - c0) * 256, 0x7fffffffL),
        0x00020000);
    // per instruction i: this lane's row in the chunk and byte in the U1 row (-1: padding)
    int urow[5], ubyte[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int u = 64 * i + lane;
        urow[i] = u / 18;
        ubyte[i] = u % 18 < 16 ? 16 * (u % 18) : -1;
    }
    [[maybe_unused]] auto dma = [&](int c) {
#if defined(__HIP_DEVICE_COMPILE__)  // (the host pass of hipcc does not know this builtin)
        unsigned char* dst = lds + R0_OFF + (c & 3) * 16 * RS0;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int col = qa + 3 + 16 * c + urow[i] - c0;
            const int voff = ubyte[i] < 0 ? -1 : col * 256 + ubyte[i];  // < 0 / past L1: out of range -> 0
            if (i < 4 || lane < 32)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(dst + 1024 * i),
                                                         16, voff, 0, 0, 0);
        }
#endif
    };
    dma(-1);
#pragma unroll 1
    for (int s = -1; s <= nch + 2; ++s) {
        if (s + 1 < nch) {
            dma(s + 1);
            asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        step_barrier();
    }
}

// NCHC > 0: the strip length as a compile-time constant (the headline's 16); 0: nch.
template <int NCHC>
__global__ __launch_bounds__(NWAVES * 64, 4) void midp_kernel(const unsigned char* __restrict__ U1, int L1, int nch_arg,
                                                               const u32x4* __restrict__ W,
                                                               const float* __restrict__ bias,
                                                               unsigned char* __restrict__ U2,
                                                               const int32_t* __restrict__ dT) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int nch = NCHC ? NCHC : nch_arg;
    const int b = blockIdx.y, qa = blockIdx.x * 16 * nch;
    if (dT) {  // speculative launch: L1 was the capacity
        L1 = 4 * dev_frames(dT, L1 / 4);
        if (qa >= L1) return;
    }
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool edge = qa < 16 || qa + 16 * nch + 16 > L1;
    unsigned char* u2row = U2 + (size_t)b * 4 * L1 * 128;
    if (w >= 8) __builtin_amdgcn_s_setprio(2);  // later layers: younger waves, the step waits for them
    else if (w >= 4) __builtin_amdgcn_s_setprio(1);
    switch (w) {
        case 0: layer_role<0, 0>(lds, qa, L1, nch, edge, W, bias, u2row, L1); break;
        case 1: layer_role<0, 1>(lds, qa, L1, nch, edge, W, bias, u2row, L1); break;
        case 2: layer_role<0, 2>(lds, qa, L1, nch, edge, W, bias, u2row, L1); break;
        case 3: layer_role<0, 3>(lds, qa, L1, nch, edge, W, bias, u2row, L1); break;
        case 4: layer_role<1, 0>(lds, qa, L1, nch, edge, W, bias, u2row, L1); break;
        case 5: layer_role<1, 1>(lds, qa, L1, nch, edge, W, bias, u2row, L1); break;
        case 6: layer_role<1, 2>(lds, qa, L1, nch, edge, W, bias, u2row, L1); break;
        case 7: layer_role<1, 3>(lds, qa, L1, nch, edge, W, bias, u2row, L1); break;
        case 8: layer_role<2, 0>(lds, qa, L1, nch, edge, W, bias, u2row, L1); break;
        case 9: layer_role<2, 1>(lds, qa, L1, nch, edge, W, bias, u2row, L1); break;
        case 10: layer_role<2, 2>(lds, qa, L1, nch, edge, W, bias, u2row, L1); break;
        case 11: layer_role<2, 3>(lds, qa, L1, nch, edge, W, bias, u2row, L1); break;
        default:
            if constexpr (MIDP_DMA) loader_role_dma(lds, qa, L1, nch, U1 + (size_t)b * L1 * 256);
            else if (edge) loader_role<true>(lds, qa, L1, nch, U1 + (size_t)b * L1 * 256);
            else loader_role<false>(lds, qa, L1, nch, U1 + (size_t)b * L1 * 256);
            break;
    }
}

static_assert(NWAVES * 64 == kMidpThreads && LDS_BYTES == kMidpLds, "the launch plan's numbers (vocoder_launch.h)");

// NCHC 16 (the headline's strip length as a compile-time constant) and 0 (nch).
template <int NCHC>
KernelRow row() {
    return {reinterpret_cast<const void*>(&midp_kernel<NCHC>), NWAVES * 64, LDS_BYTES};
}
const KernelRow kRows[2] = {row<16>(), row<0>()};  // [nch != 16]

}  // namespace mp

const char* const kVocMidpKernelName = "midp_kernel (ConvT2 + ResBlock2, pipelined)";

int32_t launch_vocoder_midp(const void* U1, int L1, int nch, const VocGrid& g, const vx_u32x4* W, const float* bias,
                            void* U2, hipStream_t st, const int32_t* dT) {
    static const hipError_t attr = set_rows_lds(mp::kRows, 2);  // once, thread-safe; a failure stays
    if (attr != hipSuccess) return hip_status(attr, "midp_kernel: hipFuncSetAttribute (one-time setup)");
    void* args[] = {&U1, &L1, &nch, &W, &bias, &U2, &dT};
    return launch_row(mp::kRows[nch != 16], g, st, args, "midp_kernel");
}

// ---------------------------------------------------------------------------
// Host packing (vocoder_pipe.h): dense polyphase matrices Wd[row][dq + 1][input
// row] (128 x 3 x 128) cut into (m-block, k-block) fragment pairs along
// mp::mslot (no m-block reads a slot twice), unscaled hi/lo halves.
bool pack_midp(const MidpSrc& s, std::vector<uint16_t>* wout, std::vector<float>* bout, bool* range_ok) {
    using namespace pipe;
    std::vector<PolyDense> d(3, PolyDense(128, 128));
    // ConvTranspose1d(64 -> 32, k 8, stride 4, pad 2), W [64][32][8]
    // (tts_model.py:255-263): out[4m + s] = x[m] W[s+2] + (s < 2 ? x[m-1] W[s+6] : x[m+1] W[s-2]).
    for (int sp = 0; sp < 4; ++sp)
        for (int co = 0; co < 32; ++co)
            for (int ci = 0; ci < 64; ++ci) {
                d[0].at(32 * sp + co, 0, ci) += s.wt[((size_t)ci * 32 + co) * 8 + sp + 2];
                if (sp < 2) d[0].at(32 * sp + co, -1, ci) += s.wt[((size_t)ci * 32 + co) * 8 + sp + 6];
                else d[0].at(32 * sp + co, 1, ci) += s.wt[((size_t)ci * 32 + co) * 8 + sp - 2];
            }
    dense_conv3(d[1], s.w1, 4, 32, 32);
    dense_conv3(d[2], s.w2, 4, 32, 32);
    wout->assign((size_t)mp::kUnits * 2 * 64 * 8, 0);
    for (int l = 0; l < 3; ++l)
        for (int mb = 0; mb < 8; ++mb)
            if (!cut_fragments(
                    d[l], mp::munit0(l) + mb * mp::mkb(l), mp::mkb(l), [&](int li) { return mb * 16 + li; },
                    [&](int kb, int g) { return mp::mslot(l, mb / 2, kb, g); }, wout, range_ok))
                return false;
    bout->assign(3 * 128, 0.f);
    const float* bsrc[3] = {s.bt, s.b1, s.b2};
    for (int l = 0; l < 3; ++l)
        for (int row = 0; row < 128; ++row) (*bout)[l * 128 + row] = bsrc[l][row % 32];
    return true;
}

}  // namespace m2
