// Fused SimpleVocoder on the f16 MFMA with a three-product split (gfx950).
//
// Same three launches and the same exact-halo windows as vocoder_fused.hip
// (head: input_conv -> ConvT1 -> ResBlock1, mid: ConvT2 -> ResBlock2, tail:
// ConvT3 -> ResBlock3 -> ConvT4 -> ResBlock4 -> output_conv -> tanh), but the
// GEMMs run on v_mfma_f32_16x16x32_f16 (16 cycles for 16K FLOP, 16x the
// FLOP rate of the f32 MFMA) with every fp32 operand x carried as two halves
//     x_hi = f16(x),  x_lo = f16(x - x_hi)        (split2u, vocoder_fused.h)
// and every product as
//     a.b ~= a_hi.b_hi + (a_hi.b_lo + a_lo.b_hi)
// accumulated in fp32 (two accumulators per tile, summed in the epilogue).
// The dropped a_lo.b_lo term is 2^-22 relative, and each half-product is
// exact in the fp32 accumulator, so the result carries fp32-level error:
// simulated over the whole stage1/stage2 vocoder (tools/probe/split_sim.py)
// the waveform RMS error vs fp64 is 3e-7 against 1.5e-7 for plain fp32
// convolution (plain f16 operands: 3.1e-4, outside the 1e-4 bound).  Three
// MFMAs per product leave 16/3 = 5.3x the exact-f32 MFMA rate.  Range: |x| and
// |w| must stay below 65504 (f16 max); weights are checked at model creation.
//
// Data layout.  Activations live position-major: one row per position holding
// hi[C] then lo[C] (f16), rows padded to a stride RS with RS/16 = 2 (mod 4) so
// the 16-lane groups of a ds_read_b128 hit 16 distinct 16-B bank quads.  An
// MFMA B fragment (lane = position j, 8 consecutive channels of one tap) is
// one ds_read_b128 for the hi half and one for the lo half.  The global
// intermediates U1 [B][4T] and U2 [B][16T] use the same row format (4*C
// bytes per position, the bytes of an fp32 tensor), so the next kernel copies
// rows without converting.  Weights are packed per (phase, m-block, k-block of
// 32) as [hi|lo][lane][8 halves]: two global_load_dwordx4 per lane.
// K order: k-block kb, lane group g = lane>>4 covers octet o = 4kb+g of the
// (tap, channel/8) sequence; any k order shared by A and B gives the same sum.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <atomic>
#include <functional>

#include "m2_common.h"
#include "vocoder_fused.h"
#include "vocoder_launch.h"
#include "vocoder_midp.h"

namespace m2 {
namespace x3 {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef vx_u32x4 u32x4;
typedef float f32x4 __attribute__((ext_vector_type(4)));


__device__ __forceinline__ f32x4 mfma_h(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
}

// An LDS activation window: rows of RS bytes, absolute position of row 0.
struct XW {
    unsigned char* p;
    int start;
};

__device__ __forceinline__ void split4(const float (&v)[4], h4& hi, h4& lo) {
    unsigned h0, h1, l0, l1;
    split2u(v[0], v[1], h0, l0);
    split2u(v[2], v[3], h1, l1);
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    hi = __builtin_bit_cast(h4, u32x2{h0, h1});
    lo = __builtin_bit_cast(h4, u32x2{l0, l1});
}

template <int CIN, int NTAP>
constexpr int nkb_of() { return (NTAP * (CIN / 8) + 3) / 4; }

// ---------------------------------------------------------------------------
// acc[n] += A_hi.B_hi + A_hi.B_lo + A_lo.B_hi over all k-blocks, for
// NT 16-position tiles (NT compile-time: no per-tile guards, which would
// make the MFMA chain conditional code and blow up register allocation).
// wp: this lane's A slot of k-block 0 (u32x4 units, k-block stride 128 =
// hi + lo).  bp: LDS row of this lane's position for tap 0 and k-block 0,
// before the lane-group offset.  Tap k reads row bp + k*STEP (STEP = +1 for
// conv3 [t-1, t, t+1], -1 for the ConvT taps).
// XR (residual fold, 8- and 16-channel ResBlock conv2): the padding octets
// of the last k-block read the block input x at the output row (xr) and the
// packed weights hold the identity there, so the GEMM itself adds x.
// NMB m-blocks (weight rows WS u32x4 apart) share every B fragment read.
// a: the weight-fragment pipeline (PD k-blocks in flight).  PRE: the caller
// already issued the loads of k-blocks 0 .. PD-1 (the previous layer's item
// did, before its epilogue and the barrier); wp_next (PD == 4, NMB == 1): once
// this item's last MFMA is issued, start the next item's first PD k-blocks.
template <int CIN, int NTAP, int NMB, int PDM = 4>
constexpr int pd_of() {
    constexpr int NKB = (NTAP * (CIN / 8) + 3) / 4;
    return NKB < PDM / NMB ? NKB : PDM / NMB;
}
// TB: tap k's rows start at tb[k] (this lane's row and lane-group chunk, the
// plane swizzle applied) instead of bp + k*STEP*RSI - the phase-planar
// layouts of the head.
// BP: see below.
template <int CIN, int NTAP, int STEP, int RSI, int NT, bool XR, int NMB, int WS, bool PRE, bool TB = false,
          int PDM = 4, int BP = 0>
__device__ __forceinline__ void mma_x3(const u32x4* __restrict__ wp, const unsigned char* bp,
                                       const unsigned char* xr, f32x4 (&acc)[NMB][NT],
                                       u32x4 (&a)[pd_of<CIN, NTAP, NMB, PDM>()][NMB][2], const u32x4* wp_next,
                                       const unsigned char* const* tb = nullptr) {
    constexpr int NOCT = CIN / 8, NK = NTAP * NOCT, NKB = (NK + 3) / 4;
    static_assert(CIN % 8 == 0 && (NOCT <= 2 || NOCT % 4 == 0), "channel count must be 8, 16 or a multiple of 32");
    static_assert(!XR || 4 * NKB - NK == NOCT, "residual fold needs exactly one row of padding octets");
    constexpr int Q = NOCT >= 4 ? 4 : NOCT;     // lane groups per tap row
    constexpr int TPK = NOCT >= 4 ? 0 : 4 / Q;  // taps per k-block when a tap row has < 4 octets
    auto koff = [](int kb) {
        const int tap = NOCT >= 4 ? kb / (NOCT / 4) : kb * TPK;
        const int col = NOCT >= 4 ? (kb % (NOCT / 4)) * 64 : 0;
        return tap * STEP * RSI + col;
    };
    const int g = (threadIdx.x & 63) >> 4;
    const unsigned char* bl = bp + (g / Q) * STEP * RSI + (g % Q) * 16;
    // Last k-block: padding octets (zero weights) re-read octet 0's bytes -
    // inside the window and finite - or, with XR, x's octet (o - NK).
    const int o_last = 4 * (NKB - 1) + g;
    const unsigned char* b_last = o_last < NK ? bl + koff(NKB - 1)
                                              : (XR ? xr + (o_last - NK) * 16 : bp + koff(NKB - 1));
    // Weight fragments stream PD k-blocks ahead (PD = all of them up to
    // PDM / NMB): one L2 round trip per item rather than one per k-block (a
    // k-block is only 3*NT*NMB MFMAs, shorter than an L2 hit), at most
    // 8 * PDM VGPRs in flight (PDM = 4 where the register budget is 128 per
    // wave, the config's PDM where it is 256: the stage2 kernels).
    constexpr int PD = pd_of<CIN, NTAP, NMB, PDM>();
    if (!PRE)
#pragma unroll
    for (int kb = 0; kb < PD; ++kb)
#pragma unroll
        for (int m = 0; m < NMB; ++m) {
            a[kb][m][0] = wp[m * WS + kb * 128];
            a[kb][m][1] = wp[m * WS + kb * 128 + 64];
        }
    auto bbase = [&](int kb) {
        if constexpr (TB) {
            static_assert(NOCT >= 4 && !XR, "tap bases: whole octet rows only");
            return tb[kb / (NOCT / 4)] + (kb % (NOCT / 4)) * 64;  // tb: the lane group's chunk included
        } else {
            return kb == NKB - 1 ? b_last : bl + koff(kb);
        }
    };
    // BP 1: k-block kb + 1's B fragments are read from LDS before k-block
    // kb's MFMAs are issued (two register buffers, 8 NT more VGPRs), so their
    // LDS latency hides behind the MFMAs instead of sitting before each
    // k-block's first; BP 2: only the hi fragments one k-block ahead (4 NT
    // more VGPRs).  Taken where it measured faster (the stage2 head, CfgS2).
    constexpr int NBH = BP ? 2 : 1, NBL = BP == 1 ? 2 : 1;
    u32x4 bh[NBH][NT], blo[NBL][NT];
    auto readh = [&](int kb, int q) {
        const unsigned char* b0 = bbase(kb);
#pragma unroll
        for (int n = 0; n < NT; ++n) bh[q][n] = *reinterpret_cast<const u32x4*>(b0 + n * 16 * RSI);
    };
    auto readl = [&](int kb, int q) {
        const unsigned char* b0 = bbase(kb);
#pragma unroll
        for (int n = 0; n < NT; ++n) blo[q][n] = *reinterpret_cast<const u32x4*>(b0 + n * 16 * RSI + 2 * CIN);
    };
    if constexpr (BP) readh(0, 0);
    if constexpr (BP == 1) readl(0, 0);
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
        const int q = BP ? (kb & 1) : 0, ql = BP == 1 ? (kb & 1) : 0;
        if constexpr (BP == 2) readl(kb, 0);
        if constexpr (BP) {
            if (kb + 1 < NKB) {
                readh(kb + 1, (kb + 1) & 1);
                if constexpr (BP == 1) readl(kb + 1, (kb + 1) & 1);
            }
        } else {
            readh(kb, 0);
            readl(kb, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < NMB; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[m][n] = mfma_h(a[kb % PD][m][0], bh[q][n], acc[m][n]);
#pragma unroll
        for (int m = 0; m < NMB; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[m][n] = mfma_h(a[kb % PD][m][0], blo[ql][n], acc[m][n]);
#pragma unroll
        for (int m = 0; m < NMB; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[m][n] = mfma_h(a[kb % PD][m][1], bh[q][n], acc[m][n]);
        if (kb + PD < NKB) {
#pragma unroll
            for (int m = 0; m < NMB; ++m) {
                a[kb % PD][m][0] = wp[m * WS + (kb + PD) * 128];
                a[kb % PD][m][1] = wp[m * WS + (kb + PD) * 128 + 64];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (PD == 4 && NMB == 1) {
        if (wp_next) {
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                a[kb][0][0] = wp_next[kb * 128];
                a[kb][0][1] = wp_next[kb * 128 + 64];
            }
        }
    }
}


// Epilogue for one tile (acc already holds the bias): v = act(acc)
// [+ residual read back from `out`], 0 outside [0, L) (only
// evaluated for tiles that reach past an edge), split and stored as hi/lo.
// Executed by every lane (the permlane16 swap reads the partner lane group);
// `store` says whether this lane's 16 B are written.  After the swap lane group
// 0 (2) holds the hi halves of channels 0-7 (8-15) of the m-block and group 1
// (3) the lo halves: one ds_write_b128 per lane instead of two ds_write_b64
// (2-way instead of 4-way bank conflicts on RS/16 = 2 mod 4 rows).
// GO: the tile goes straight to global rows of 4*COUT bytes (gout, absolute
// position t, t < L only) instead of back into `out` (the residual is still
// read from `out`).
template <int COUT, int RSO, int ACT, bool RES, bool GO>
__device__ __forceinline__ void store_tile(const f32x4& acc, XW out, int t, int co0, int L,
                                           bool edge, bool store, unsigned char* gout) {
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = acc[r];
    if constexpr (ACT == ACT_LEAKY) leaky4(v);
    else static_assert(ACT == ACT_NONE, "x3 layers: leaky or none");
    unsigned char* rowp = out.p + (t - out.start) * RSO;
    if (RES) {
        const unsigned char* row = rowp + co0 * 2;
        const h4 hi = *reinterpret_cast<const h4*>(row), lo = *reinterpret_cast<const h4*>(row + 2 * COUT);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += (float)hi[r] + (float)lo[r];
    }
    if (!GO && edge && (t < 0 || t >= L)) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = 0.f;
    }
    unsigned h0, h1, l0, l1;
    split2u(v[0], v[1], h0, l0);
    split2u(v[2], v[3], h1, l1);
    const auto s0 = __builtin_amdgcn_permlane16_swap(h0, l0, false, false);
    const auto s1 = __builtin_amdgcn_permlane16_swap(h1, l1, false, false);
    const int g = (threadIdx.x & 63) >> 4;
    const int off = 2 * (co0 - 4 * g + 8 * (g >> 1)) + (g & 1) * 2 * COUT;
    if constexpr (GO) {
        if (store && t < L)
            *reinterpret_cast<u32x4*>(gout + (size_t)t * 4 * COUT + off) = u32x4{s0[0], s1[0], s0[1], s1[1]};
    } else if (store) {
        *reinterpret_cast<u32x4*>(rowp + off) = u32x4{s0[0], s1[0], s0[1], s1[1]};
    }
}

// Does 3-tap packing fold the ResBlock residual into the GEMM (see mma_x3)?
// Must agree with the host packer (res_fold_channels in vocoder_fused.h).
template <int C>
constexpr bool kFold = res_fold_channels(C);

// One work item: NTT tiles of NMB (phase, m-block) rows (consecutive m-blocks
// of one phase, co0 .. co0 + 16 NMB, sharing the B fragments) starting at
// tile0.  Output position of column j (relative to the layer's first input
// q0 / a0): t = (p0 + j) * RR + ph (RR = 1, ph = 0 for conv3).
// corr (the composed stage2 head): per-(phase, channel) terms subtracted from
// the outputs of input column qe (an utterance edge), before the activation.
template <int CIN, int COUT, int NTAP, int STEP, int RSI, int RSO, int NTT, int ACT, bool RES, bool XR, int RR,
          int JMAX, int NMB, bool PRE, bool GO = false, int PDM = 4, int BP = 0>
__device__ __forceinline__ void run_item(const u32x4* __restrict__ wp, const float* __restrict__ bias,
                                         const unsigned char* bp, const unsigned char* xr, XW out, int co0, int p0,
                                         int ph, int tile0, int L, u32x4 (&a)[pd_of<CIN, NTAP, NMB, PDM>()][NMB][2],
                                         const u32x4* wp_next, unsigned char* gout = nullptr,
                                         const unsigned char* corr = nullptr, int qe = 0) {
    constexpr int WS = nkb_of<CIN, NTAP>() * 128;  // u32x4 between consecutive m-blocks' weights
    f32x4 acc[NMB][NTT];
#pragma unroll
    for (int m = 0; m < NMB; ++m) {
        f32x4 bv;
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[r] = co0 + 16 * m + r < COUT ? bias[co0 + 16 * m + r] : 0.f;
#pragma unroll
        for (int n = 0; n < NTT; ++n) acc[m][n] = bv;
    }
    mma_x3<CIN, NTAP, STEP, RSI, NTT, XR, NMB, WS, PRE, false, PDM, BP>(wp, bp, xr, acc, a, wp_next);
    const bool edge = (p0 + tile0 * 16) * RR < 0 || (p0 + (tile0 + NTT) * 16) * RR > L;
    const int li = threadIdx.x & 15, g = (threadIdx.x & 63) >> 4;
    if (corr) {  // wave-uniform
#pragma unroll
        for (int n = 0; n < NTT; ++n)
            if (qe >= p0 + (tile0 + n) * 16 && qe < p0 + (tile0 + n) * 16 + 16 && p0 + (tile0 + n) * 16 + li == qe) {
#pragma unroll
                for (int m = 0; m < NMB; ++m) {
                    const f32x4 c = *reinterpret_cast<const f32x4*>(corr + 4 * (ph * COUT + co0 + 16 * m));
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[m][n][r] -= c[r];
                }
            }
    }
#pragma unroll
    for (int m = 0; m < NMB; ++m) {
        const int cm = co0 + 16 * m;
        const bool rows_ok = cm - 4 * g + 8 * (g >> 1) < COUT;  // after the swap: this lane's 8 channels
#pragma unroll
        for (int n = 0; n < NTT; ++n) {
            const int j = (tile0 + n) * 16 + li;
            const bool col_ok = ((tile0 + n + 1) * 16 <= JMAX) || j < JMAX;
            store_tile<COUT, RSO, ACT, RES, GO>(acc[m][n], out, (p0 + j) * RR + ph, cm, L, edge, rows_ok && col_ok,
                                                gout);
        }
    }
}

// Work items of a layer: (row, chunk) with each row's NTILES split into
// NCH = ceil(NTILES / NT) chunks whose sizes differ by at most one tile
// (25 tiles, NT 4: seven chunks of 3-4 rather than six of 4 and one of 1),
// dealt round-robin over the waves.  Chunk sizes are compile-time (QLO or
// QLO + 1): two instantiations of the item body, no per-tile guards.
template <int NTILES, int NT>
struct Chunks {
    static constexpr int NCH = (NTILES + NT - 1) / NT, QLO = NTILES / NCH, QHI = QLO + (NTILES % NCH ? 1 : 0);
    __device__ static int lo(int k) { return k * NTILES / NCH; }
};

// Weight-fragment hand-off between the layers of a kernel in which every wave
// does exactly one item per layer (the stage1 head): the loads of the next
// layer's first four k-blocks are issued right after the current item's last
// MFMA, so they are in flight during its epilogue and the barrier.
typedef u32x4 APipe[4][1][2];

// Work items of a layer: (m-block group, chunk) for conv3, (phase, m-block
// group, chunk) for the transposed convs; NMB m-blocks per item share the B
// reads.  ONE (= the wave count, one item each): the wave's item is its index, its
// first k-blocks' weights were loaded into `ap` by the previous layer, and it
// starts the loads of `wp_next` (the next layer's item) into `ap`.
template <int CIN, int COUT, int NT, int NPOS, int NMB>
struct Conv3Items {
    static constexpr int MB = (COUT + 15) / 16, NKB = nkb_of<CIN, 3>(), MG = MB / NMB;
    static_assert(MB % NMB == 0, "m-block groups");
    using CH = Chunks<(NPOS + 15) / 16, NT>;
    static constexpr int N = MG * CH::NCH;
    __device__ static const u32x4* wp(const u32x4* Wp, int item) {
        return Wp + (size_t)(item % MG) * NMB * NKB * 128 + (threadIdx.x & 63);
    }
};
template <int CIN, int COUT, int R, int NT, int NQ, int NMB>
struct ConvTItems {
    static constexpr int MB = (COUT + 15) / 16, NKB = nkb_of<CIN, 2>(), MG = MB / NMB;
    static_assert(MB % NMB == 0, "m-block groups");
    using CH = Chunks<(NQ + 15) / 16, NT>;
    static constexpr int N = R * MG * CH::NCH;
    __device__ static const u32x4* wp(const u32x4* Wp, int item) {
        const int rg = item % (R * MG), ph = rg / MG, mb = (rg - ph * MG) * NMB;
        return Wp + (size_t)(ph * MB + mb) * NKB * 128 + (threadIdx.x & 63);
    }
};

// Conv1d(k=3, pad=1): abs positions [a0, a0+NPOS) of `out` from `in`.
// RES: out += conv(in) (ResBlock conv2, x = out), folded into the GEMM for
// 8/16 channels, read back in the epilogue otherwise.
// GO: store the output tiles to global rows (gout) instead of `out`.
template <int CIN, int COUT, int NT, int ACT, bool RES, int RSI, int RSO, int NPOS, int NMB = 1, int ONE = 0,
          bool GO = false, int PDM = 4, int BP = 0>
__device__ __forceinline__ void xconv3(const u32x4* __restrict__ Wp, const float* __restrict__ bias, XW in, XW out,
                                       int a0, int L, APipe* ap = nullptr, const u32x4* wp_next = nullptr,
                                       unsigned char* gout = nullptr) {
    using IT = Conv3Items<CIN, COUT, NT, NPOS, NMB>;
    using CH = typename IT::CH;
    constexpr int MG = IT::MG;
    constexpr bool FOLD = RES && kFold<CIN>;
    static_assert(!FOLD || (CIN == COUT && RSI == RSO), "folded residual: x has the conv's input layout");
    static_assert(!ONE || (IT::N == ONE && NMB == 1 && pd_of<CIN, 3, 1>() == 4), "one item per wave");
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
    auto body = [&](int item, auto pre) {
        constexpr bool PRE = decltype(pre)::value;
        const int mb = (item % MG) * NMB, k = item / MG;
        const int tile0 = CH::lo(k), nt = CH::lo(k + 1) - tile0;
        const int co0 = mb * 16 + 4 * g;
        const int p = a0 + tile0 * 16 + li;  // this lane's output position in tile 0
        const u32x4* wp = IT::wp(Wp, item);
        const unsigned char* bp = in.p + (p - 1 - in.start) * RSI;
        const unsigned char* xr = out.p + (p - out.start) * RSO;
        u32x4 al[pd_of<CIN, 3, NMB, PDM>()][NMB][2];
        auto& a = [&]() -> auto& {
            if constexpr (PRE) return *ap;
            else return al;
        }();
        if (nt == CH::QHI)
            run_item<CIN, COUT, 3, 1, RSI, RSO, CH::QHI, ACT, RES && !FOLD, FOLD, 1, NPOS, NMB, PRE, GO, PDM, BP>(
                wp, bias, bp, xr, out, co0, a0, 0, tile0, L, a, wp_next, gout);
        else
            run_item<CIN, COUT, 3, 1, RSI, RSO, CH::QLO, ACT, RES && !FOLD, FOLD, 1, NPOS, NMB, PRE, GO, PDM, BP>(
                wp, bias, bp, xr, out, co0, a0, 0, tile0, L, a, wp_next, gout);
    };
    if constexpr (ONE) {
        body(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), std::true_type{});
    } else {
#pragma unroll 1
        for (int item = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); item < IT::N; item += blockDim.x >> 6)
            body(item, std::false_type{});
    }
}

// leaky(ConvTranspose1d(k=2R, stride R, pad R/2)): inputs q in [q0, q0+NQ)
// give outputs t = q*R + ph.  Phase ph reads taps (q, q-1) if ph + R/2 < R,
// else (q+1, q): B base row q + d0, tap k at row q + d0 - k.
template <int CIN, int COUT, int R, int NT, int RSI, int RSO, int NQ, int NMB = 1, int ONE = 0, int PDM = 4>
__device__ __forceinline__ void xconvT(const u32x4* __restrict__ Wp, const float* __restrict__ bias, XW in, XW out,
                                       int q0, int L, APipe* ap = nullptr, const u32x4* wp_next = nullptr) {
    using IT = ConvTItems<CIN, COUT, R, NT, NQ, NMB>;
    using CH = typename IT::CH;
    constexpr int MG = IT::MG, PAD = R / 2;
    static_assert(!ONE || (IT::N == ONE && NMB == 1 && pd_of<CIN, 2, 1>() == 4), "one item per wave");
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
    auto body = [&](int item, auto pre) {
        constexpr bool PRE = decltype(pre)::value;
        const int rg = item % (R * MG), k = item / (R * MG);  // rg = ph*MG + m-block group
        const int ph = rg / MG, mb = (rg - ph * MG) * NMB;
        const int tile0 = CH::lo(k), nt = CH::lo(k + 1) - tile0;
        const int d0 = (ph + PAD < R) ? 0 : 1;
        const int co0 = mb * 16 + 4 * g;
        const u32x4* wp = IT::wp(Wp, item);
        const unsigned char* bp = in.p + (q0 + tile0 * 16 + li + d0 - in.start) * RSI;
        u32x4 al[pd_of<CIN, 2, NMB, PDM>()][NMB][2];
        auto& a = [&]() -> auto& {
            if constexpr (PRE) return *ap;
            else return al;
        }();
        if (nt == CH::QHI)
            run_item<CIN, COUT, 2, -1, RSI, RSO, CH::QHI, ACT_LEAKY, false, false, R, NQ, NMB, PRE, false, PDM>(
                wp, bias, bp, nullptr, out, co0, q0, ph, tile0, L, a, wp_next);
        else
            run_item<CIN, COUT, 2, -1, RSI, RSO, CH::QLO, ACT_LEAKY, false, false, R, NQ, NMB, PRE, false, PDM>(
                wp, bias, bp, nullptr, out, co0, q0, ph, tile0, L, a, wp_next);
    };
    if constexpr (ONE) {
        body(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), std::true_type{});
    } else {
#pragma unroll 1
        for (int item = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); item < IT::N; item += blockDim.x >> 6)
            body(item, std::false_type{});
    }
}

// The composed input_conv o ConvT1 on the generic item path (the stage2
// head): head_convT1c_planar's layer over (phase, m-block, chunk) items, 4
// mel taps (frames q + d0 + 1 - k), per-phase bias, edge terms from `corr`.
template <int MP, int COUT, int NT, int RSI, int RSO, int NQ, int PDM = 4, int BP = 0>
__device__ __forceinline__ void xconvT1c(const u32x4* __restrict__ Wp, const float* __restrict__ bias,
                                         const unsigned char* corr, XW mel, XW out, int q0, int T) {
    constexpr int R = 4, MB = (COUT + 15) / 16, NKB = nkb_of<MP, 4>();
    using CH = Chunks<(NQ + 15) / 16, NT>;
    constexpr int N = R * MB * CH::NCH;
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
#pragma unroll 1
    for (int item = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); item < N; item += blockDim.x >> 6) {
        const int rg = item % (R * MB), k = item / (R * MB), ph = rg / MB, mb = rg - ph * MB;
        const int tile0 = CH::lo(k), nt = CH::lo(k + 1) - tile0, d0 = ph < 2 ? 0 : 1, co0 = mb * 16 + 4 * g;
        const u32x4* wp = Wp + (size_t)(ph * MB + mb) * NKB * 128 + lane;
        const unsigned char* bp = mel.p + (q0 + tile0 * 16 + li + d0 + 1 - mel.start) * RSI;
        const int qe = ph < 2 ? 0 : T - 1;
        u32x4 al[pd_of<MP, 4, 1, PDM>()][1][2];
        if (nt == CH::QHI)
            run_item<MP, COUT, 4, -1, RSI, RSO, CH::QHI, ACT_LEAKY, false, false, R, NQ, 1, false, false, PDM, BP>(
                wp, bias + ph * COUT, bp, nullptr, out, co0, q0, ph, tile0, 4 * T, al, nullptr, nullptr, corr, qe);
        else
            run_item<MP, COUT, 4, -1, RSI, RSO, CH::QLO, ACT_LEAKY, false, false, R, NQ, 1, false, false, PDM, BP>(
                wp, bias + ph * COUT, bp, nullptr, out, co0, q0, ph, tile0, 4 * T, al, nullptr, nullptr, corr, qe);
    }
}

// Edge terms of the composed stage2 head: thread v (4 x COUT threads) sums
// E[v][0..M) . mel[edge] + e[v] into corr (the windows holding an edge only).
template <int M, int MP, int COUT, int RSM>
__device__ __forceinline__ void head_edge_terms_s2(const float* __restrict__ hce, XW mel, int T, bool left,
                                                   bool right, unsigned char* corr) {
    const int v = threadIdx.x, ph = v / COUT;
    if (v >= 4 * COUT) return;
    const bool need = ph < 2 ? left : right;
    float d = 0.f;
    if (need) {
        const unsigned char* row = mel.p + ((ph < 2 ? 0 : T - 1) - mel.start) * RSM;
        d = hce[4 * COUT * MP + v];
#pragma unroll
        for (int o = 0; o < M / 8; ++o) {
            const h8 hi = *reinterpret_cast<const h8*>(row + 16 * o);
            const h8 lo = *reinterpret_cast<const h8*>(row + 2 * MP + 16 * o);
            const float4 e0 = *reinterpret_cast<const float4*>(hce + (size_t)v * MP + 8 * o);
            const float4 e1 = *reinterpret_cast<const float4*>(hce + (size_t)v * MP + 8 * o + 4);
            const float e[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
#pragma unroll
            for (int i = 0; i < 8; ++i) d = fmaf(e[i], (float)hi[i] + (float)lo[i], d);
        }
    }
    *reinterpret_cast<float*>(corr + 4 * v) = d;
}

// ---------------------------------------------------------------------------
// Phase-planar head (stage1, one item per wave).  ConvT1's output u (x4) and
// ResBlock1's hidden h are kept as 4 planes of 64 rows, plane p = positions
// t = 4q + p for q in [qs(p), qs(p) + 64): u: qs = f0 - 1 for p >= 2, else
// f0; h: qs = f0 - 1 for p = 3, else f0 - exactly the positions the next
// layer reads.  Against the position-major layout (ConvT1 NQ = 65 inputs =
// 5 tiles per phase, outputs 4 rows apart) this is 4 tiles per phase (20 %
// fewer ConvT1 MFMAs) and conflict-free epilogue stores (consecutive lanes,
// consecutive rows); the ResBlock1 convs become per-phase GEMMs whose three
// taps read rows of the neighbouring planes (mma_x3 with tap bases).
// Plane rows are swizzled: row r's 16-B chunks c and c ^ 1 trade places when
// bit 2 of r is set (plane_sw).  A tile's epilogue writes rows li of one
// chunk per lane group, 8 consecutive lanes per ds_write_b128 pass; at a row
// stride of 18 chunks rows r and r + 4 met in the same banks (2-way); the
// swizzle moves rows 4-7 by 4 banks.  The B-fragment reads (4 lane groups
// of 16, chunks c0 + g) stay conflict-free: the bit only permutes the chunk
// pairs of one k-block, per lane, and folds into the tap bases.
__device__ __forceinline__ int plane_sw(int r) { return (r >> 2) & 1; }
__device__ __forceinline__ int qs_u(int p, int f0) { return f0 - (p >= 2 ? 1 : 0); }
__device__ __forceinline__ int qs_h(int p, int f0) { return f0 - (p == 3 ? 1 : 0); }
constexpr int kPlane = 64;

// Epilogue of one tile into an explicit plane row (rowp, swizzle bit rsw) or
// straight to global (GO); the residual, if any, is read from plane row xrow
// (swizzle bit xsw).
template <int COUT, int ACT, bool RES, bool GO>
__device__ __forceinline__ void store_row(const f32x4& acc, unsigned char* rowp, const unsigned char* xrow, int co0,
                                          bool zero, bool store, unsigned char* gout, int t, int rsw, int xsw = 0) {
    const int g = (threadIdx.x & 63) >> 4;
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = acc[r];
    if constexpr (ACT == ACT_LEAKY) leaky4(v);
    if constexpr (RES) {  // channels co0 .. co0 + 3: chunk co0 / 8, half g & 1
        const unsigned char* row = xrow + 2 * (co0 - 4 * g) + 16 * ((g >> 1) ^ xsw) + 8 * (g & 1);
        const h4 hi = *reinterpret_cast<const h4*>(row), lo = *reinterpret_cast<const h4*>(row + 2 * COUT);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += (float)hi[r] + (float)lo[r];
    }
    if (zero) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = 0.f;
    }
    unsigned h0, h1, l0, l1;
    split2u(v[0], v[1], h0, l0);
    split2u(v[2], v[3], h1, l1);
    const auto s0 = __builtin_amdgcn_permlane16_swap(h0, l0, false, false);
    const auto s1 = __builtin_amdgcn_permlane16_swap(h1, l1, false, false);
    const int off = 2 * (co0 - 4 * g) + (g & 1) * 2 * COUT;
    if (store) {
        if constexpr (GO)
            *reinterpret_cast<u32x4*>(gout + (size_t)t * 4 * COUT + off + 16 * (g >> 1)) =
                u32x4{s0[0], s1[0], s0[1], s1[1]};
        else
            *reinterpret_cast<u32x4*>(rowp + off + 16 * ((g >> 1) ^ rsw)) = u32x4{s0[0], s1[0], s0[1], s1[1]};
    }
}

// ConvT1 (x4, k 8, pad 2) + leaky from the position-major inconv output (in,
// frames f0-2 ..) into the u planes; item = wave = (phase, m-block).
template <int CIN, int COUT, int RSI, int RSO>
__device__ __forceinline__ void head_convT1_planar(const u32x4* __restrict__ Wp, const float* __restrict__ bias,
                                                   XW in, unsigned char* u, int f0, int L, APipe* ap,
                                                   const u32x4* wp_next) {
    constexpr int MB = COUT / 16, NKB = nkb_of<CIN, 2>(), NT = 4;
    const int item = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ph = item / MB, mb = item - ph * MB;
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4, co0 = mb * 16 + 4 * g;
    const int qs = qs_u(ph, f0), d0 = ph < 2 ? 0 : 1;  // taps (q + d0, q + d0 - 1)
    const u32x4* wp = Wp + (size_t)(ph * MB + mb) * NKB * 128 + lane;
    const unsigned char* bp = in.p + (qs + li + d0 - in.start) * RSI;
    f32x4 acc[1][NT];
    f32x4 bv;
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[r] = bias[co0 + r];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[0][n] = bv;
    mma_x3<CIN, 2, -1, RSI, NT, false, 1, NKB * 128, true>(wp, bp, nullptr, acc, *ap, wp_next);
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int t = 4 * (qs + 16 * n + li) + ph;
        store_row<COUT, ACT_LEAKY, false, false>(acc[0][n], u + (ph * kPlane + 16 * n + li) * RSO, nullptr, co0,
                                                 t < 0 || t >= L, true, nullptr, t, plane_sw(li));
    }
}

// input_conv composed into ConvT1 (stage1 head, round 2): the input conv
// (k3, no activation) feeds only ConvT1, which is linear before its leaky, so
// u = leaky(Wc * mel + bc[ph]) with Wc[ph] = W_T[ph] o W_in a 4-tap transposed
// conv straight from the mel window (output phase ph at input column q reads
// mel frames q + d0 + 1 - k, k = 0..3, d0 = 0 for ph < 2 else 1): K = 4 x 64
// mel channels, the same 8 k-blocks as ConvT1's 2 x 128, and no input-conv
// layer (its MFMAs, barrier and LDS round trip) at all.  The reference's
// ConvT1 sees zeros at input frames -1 and T, where the composed form sees
// the input conv of the zero-padded mel (b_in + W_in[.,.,2] mel[0] /
// b_in + W_in[.,.,0] mel[T-1]); outputs t = 0, 1 and 4T - 2, 4T - 1 subtract
// that term: E[ph][co][m] . mel[edge] + e[ph][co] (hce: [4][C1][MP] then
// [4][C1], fp32; phases 0, 1 left edge, 2, 3 right edge).  The edge windows
// of an utterance compute those 256 sums cooperatively before the layer
// (head_edge_terms: their table loads issued at kernel start) into an LDS
// table `corr` that the lanes holding the edge outputs read (null elsewhere).
// (A per-lane loop over the table in the epilogue made the edge windows the
// kernel's critical path.)  Bias bc: [4][C1] (it depends on the phase).
// The composed head's edge terms, all 1024 threads of an edge window: thread
// t sums 16 of the 64 products of value v = t / 4 (= ph * COUT + co); four
// adjacent lanes reduce by shuffles.  ev: this thread's 16 table entries,
// loaded at kernel start (head_edge_load).
template <int MP, int COUT>
__device__ __forceinline__ void head_edge_load(const float* __restrict__ hce, float4 (&ev)[4], float& eb) {
    static_assert(4 * COUT * 4 == 1024 && MP == 64, "1024 threads: 4 phases x COUT values x 4 parts of 16");
    const int t = threadIdx.x, v = t >> 2, part = t & 3;
#pragma unroll
    for (int i = 0; i < 4; ++i) ev[i] = *reinterpret_cast<const float4*>(hce + (size_t)v * MP + 16 * part + 4 * i);
    eb = hce[4 * COUT * MP + v];
}
template <int MP, int COUT, int RSM>
__device__ __forceinline__ void head_edge_terms(const float4 (&ev)[4], float eb, XW mel, int T, bool left, bool right,
                                                unsigned char* corr) {
    const int t = threadIdx.x, v = t >> 2, part = t & 3, ph = v / COUT;
    const bool need = ph < 2 ? left : right;  // wave-uniform (16 waves, 4 per phase)
    float d = 0.f;
    if (need) {
        const unsigned char* row = mel.p + ((ph < 2 ? 0 : T - 1) - mel.start) * RSM + 2 * 16 * part;
        const float e[16] = {ev[0].x, ev[0].y, ev[0].z, ev[0].w, ev[1].x, ev[1].y, ev[1].z, ev[1].w,
                             ev[2].x, ev[2].y, ev[2].z, ev[2].w, ev[3].x, ev[3].y, ev[3].z, ev[3].w};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const h8 hi = *reinterpret_cast<const h8*>(row + 16 * h);
            const h8 lo = *reinterpret_cast<const h8*>(row + 2 * MP + 16 * h);
#pragma unroll
            for (int i = 0; i < 8; ++i) d = fmaf(e[8 * h + i], (float)hi[i] + (float)lo[i], d);
        }
    }
    d += __shfl_xor(d, 1);
    d += __shfl_xor(d, 2);
    if (part == 0) *reinterpret_cast<float*>(corr + 4 * v) = need ? d + eb : 0.f;
}

template <int MP, int COUT, int RSM, int RSO>
__device__ __forceinline__ void head_convT1c_planar(const u32x4* __restrict__ Wp, const float* __restrict__ bias,
                                                    const unsigned char* corr, XW mel, unsigned char* u, int f0,
                                                    int T, APipe* ap, const u32x4* wp_next, int rot = 0) {
    constexpr int MB = COUT / 16, NKB = nkb_of<MP, 4>(), NT = 4;
    static_assert(NKB == 8 && pd_of<MP, 4, 1>() == 4, "the ConvT1 weight pipeline shape");
    const int item = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pv = item / MB, mb = item - pv * MB;
    // rot (headmid_kernel): the window starts at position 4 f0 + rot, so plane
    // pv holds output phase (pv + rot) mod 4 of the columns one further on
    // where pv + rot wraps; the arithmetic of a position is the same
    const int ph = (pv + rot) & 3;
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4, co0 = mb * 16 + 4 * g;
    const int qs = qs_u(pv, f0) + ((pv + rot) >> 2), d0 = ph < 2 ? 0 : 1;  // taps: mel frames q + d0 + 1 - k
    const u32x4* wp = Wp + (size_t)(ph * MB + mb) * NKB * 128 + lane;
    const unsigned char* bp = mel.p + (qs + li + d0 + 1 - mel.start) * RSM;
    f32x4 acc[1][NT];
    f32x4 bv;
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[r] = bias[ph * COUT + co0 + r];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[0][n] = bv;
    mma_x3<MP, 4, -1, RSM, NT, false, 1, NKB * 128, true>(wp, bp, nullptr, acc, *ap, wp_next);
    const int L = 4 * T, qe = ph < 2 ? 0 : T - 1;  // the input column of this phase's edge outputs
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int q = qs + 16 * n + li, t = 4 * q + ph;
        if (corr && qe >= qs + 16 * n && qe < qs + 16 * n + 16) {  // wave-uniform: a tile with an edge output
            if (q == qe) {
                const f32x4 c = *reinterpret_cast<const f32x4*>(corr + 4 * (ph * COUT + co0));
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[0][n][r] -= c[r];
            }
        }
        store_row<COUT, ACT_LEAKY, false, false>(acc[0][n], u + (pv * kPlane + 16 * n + li) * RSO, nullptr, co0,
                                                 t < 0 || t >= L, true, nullptr, t, plane_sw(li));
    }
}

// ResBlock1 conv (k3, pad 1) between planes: input planes start at qsi(p),
// output plane p covers q in [qso(p), +64).  CONV2: + x from the u planes,
// stored straight to U1 (t < L and q < f0 + tf only); else leaky into the
// h planes (0 outside [0, L)).  INPL (headmid_kernel): conv2 + x goes back
// into the u planes instead, 0 outside [0, L): each lane reads the residual
// of its four channels before the permlane16 swap and writes, after it, 16 B
// of the same row and m-block, which only this wave touches.  rot: plane p
// holds positions 4 q + p + rot (head_convT1c_planar).
// Item map (wave-uniform; M2_HEAD_ITEMS, default 1 = mbmajor): the weights do
// not depend on the plane, so the four waves of an m-block load the same
// fragments.  mbmajor: they are waves 4 mb .. 4 mb + 3, one on every SIMD and
// of one age, so their loads meet in L1; else (the ConvT1 map, whose
// fragments are all distinct) waves mb, mb + 4, .. of one SIMD, which run by
// age, far apart in time, and each fetch their own copy from L2.  The sums of
// an item and their order are the same under both maps.
template <int MB>
__device__ __forceinline__ int rb1_mb(int wv, bool mbmajor) {
    return mbmajor ? wv / 4 : wv % MB;
}
template <int C, int RS, bool CONV2, bool INPL = false>
__device__ __forceinline__ void head_rb1_planar(const u32x4* __restrict__ Wp, const float* __restrict__ bias,
                                                const unsigned char* in, unsigned char* out,
                                                const unsigned char* x, int f0, int tf, int L, APipe* ap,
                                                const u32x4* wp_next, unsigned char* gout, int rot = 0,
                                                bool mbmajor = false) {
    constexpr int MB = C / 16, NKB = nkb_of<C, 3>(), NT = 4;
    static_assert(CONV2 || !INPL, "in place: conv2 only");
    const int item = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int p = mbmajor ? item % 4 : item / MB, mb = rb1_mb<MB>(item, mbmajor);
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4, co0 = mb * 16 + 4 * g;
    const int qo = CONV2 ? f0 : qs_h(p, f0);
    const unsigned char* tb[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const int pd = p + d - 1, dq = pd < 0 ? -1 : (pd > 3 ? 1 : 0), pi = pd - 4 * dq;
        const int qsi = CONV2 ? qs_h(pi, f0) : qs_u(pi, f0);
        const int r = qo + dq - qsi + li;  // row in plane pi (>= 0)
        tb[d] = in + (pi * kPlane + r) * RS + 16 * (g ^ plane_sw(r));
    }
    const u32x4* wp = Wp + (size_t)mb * NKB * 128 + lane;
    f32x4 acc[1][NT];
    f32x4 bv;
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[r] = bias[co0 + r];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[0][n] = bv;
    mma_x3<C, 3, 1, RS, NT, false, 1, NKB * 128, true, true>(wp, nullptr, nullptr, acc, *ap, wp_next, tb);
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int q = qo + 16 * n + li, t = 4 * q + p + rot;
        if constexpr (INPL) {
            const int xr = q - qs_u(p, f0);
            unsigned char* xrow = const_cast<unsigned char*>(x) + (p * kPlane + xr) * RS;
            store_row<C, ACT_NONE, true, false>(acc[0][n], xrow, xrow, co0, t < 0 || t >= L, q < f0 + tf, nullptr, t,
                                                plane_sw(xr), plane_sw(xr));
        } else if constexpr (CONV2) {
            const int xr = q - qs_u(p, f0);
            store_row<C, ACT_NONE, true, true>(acc[0][n], nullptr, x + (p * kPlane + xr) * RS, co0, false,
                                               q < f0 + tf && t < L, gout, t, 0, plane_sw(xr));
        } else {
            store_row<C, ACT_LEAKY, false, false>(acc[0][n], out + (p * kPlane + 16 * n + li) * RS, nullptr, co0,
                                                  t < 0 || t >= L, true, nullptr, t, plane_sw(li));
        }
    }
}

// ---------------------------------------------------------------------------
// Global <-> LDS.  Trip counts are compile-time (NTHR threads, N rows) so
// every thread issues all its global loads before the first LDS store.
// mel -> window rows [0, N) (abs start + r), MP channels (zero past M).
template <bool TRANS, int M, int MP, int RS, int N, int NTHR>
__device__ __forceinline__ void gload_mel(const float* __restrict__ g, int T, XW dst) {
    if (TRANS) {  // [T][M]: an item = 8 channels of one frame (two 16-B loads); consecutive threads take
                  // consecutive frames, so the LDS stores are the [M][T] branch's b128 pattern (was 16
                  // threads per frame row with 8-B hi / lo stores: [B,T,M] 0.2 us/step behind [B,M,T] in
                  // tools/probe/mel_layout_ab.py, now level)
        constexpr int OCT = MP / 8, TOT = N * OCT, IT = (TOT + NTHR - 1) / NTHR;
        float4 x[IT][2];
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const int i = threadIdx.x + k * NTHR;
            const int o = i / N, r = i - o * N, t = dst.start + r;
            const bool in = i < TOT && t >= 0 && t < T;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c = 8 * o + 4 * h;
                x[k][h] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (in && c < M) x[k][h] = *reinterpret_cast<const float4*>(g + (size_t)t * M + c);
            }
        }
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const int i = threadIdx.x + k * NTHR;
            if (i < TOT) {
                const int o = i / N, r = i - o * N;
                unsigned hh[4], ll[4];
                split2u(x[k][0].x, x[k][0].y, hh[0], ll[0]);
                split2u(x[k][0].z, x[k][0].w, hh[1], ll[1]);
                split2u(x[k][1].x, x[k][1].y, hh[2], ll[2]);
                split2u(x[k][1].z, x[k][1].w, hh[3], ll[3]);
                unsigned char* row = dst.p + r * RS + 16 * o;
                *reinterpret_cast<u32x4*>(row) = u32x4{hh[0], hh[1], hh[2], hh[3]};
                *reinterpret_cast<u32x4*>(row + 2 * MP) = u32x4{ll[0], ll[1], ll[2], ll[3]};
            }
        }
    } else {  // [M][T]: an item = 8 channels of one frame; consecutive threads take consecutive frames
        constexpr int OCT = MP / 8, TOT = N * OCT, IT = (TOT + NTHR - 1) / NTHR;
        float x[IT][8];
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const int i = threadIdx.x + k * NTHR;
            const int o = i / N, r = i - o * N, t = dst.start + r;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int c = 8 * o + e;
                x[k][e] = (i < TOT && t >= 0 && t < T && c < M) ? g[(size_t)c * T + t] : 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const int i = threadIdx.x + k * NTHR;
            if (i < TOT) {
                const int o = i / N, r = i - o * N;
                unsigned hh[4], ll[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) split2u(x[k][2 * e], x[k][2 * e + 1], hh[e], ll[e]);
                unsigned char* row = dst.p + r * RS + 16 * o;
                *reinterpret_cast<u32x4*>(row) = u32x4{hh[0], hh[1], hh[2], hh[3]};
                *reinterpret_cast<u32x4*>(row + 2 * MP) = u32x4{ll[0], ll[1], ll[2], ll[3]};
            }
        }
    }
}

// rows of 4C bytes (hi|lo) at global positions [start, start+N), zero outside [0, Lg)
template <int C, int RS, int N, int NTHR>
__device__ __forceinline__ void gload_rows(const unsigned char* __restrict__ g, int Lg, XW dst) {
    constexpr int Q = C / 4, TOT = N * Q, IT = (TOT + NTHR - 1) / NTHR;  // 16-B chunks
    u32x4 v[IT];
#pragma unroll
    for (int k = 0; k < IT; ++k) {
        const int i = threadIdx.x + k * NTHR;
        const int r = i / Q, q = i - r * Q, t = dst.start + r;
        v[k] = u32x4{0u, 0u, 0u, 0u};
        if (i < TOT && t >= 0 && t < Lg) v[k] = *reinterpret_cast<const u32x4*>(g + (size_t)t * 4 * C + q * 16);
    }
#pragma unroll
    for (int k = 0; k < IT; ++k) {
        const int i = threadIdx.x + k * NTHR;
        const int r = i / Q, q = i - r * Q;
        if (i < TOT) *reinterpret_cast<u32x4*>(dst.p + r * RS + q * 16) = v[k];
    }
}

template <int C, int RS, int N, int NTHR>
__device__ __forceinline__ void gstore_rows(unsigned char* __restrict__ g, int Lg, XW src, int a0) {
    constexpr int Q = C / 4, TOT = N * Q, IT = (TOT + NTHR - 1) / NTHR;
#pragma unroll
    for (int k = 0; k < IT; ++k) {
        const int i = threadIdx.x + k * NTHR;
        const int r = i / Q, q = i - r * Q, t = a0 + r;
        if (i < TOT && t < Lg)
            *reinterpret_cast<u32x4*>(g + (size_t)t * 4 * C + q * 16) =
                *reinterpret_cast<const u32x4*>(src.p + (t - src.start) * RS + q * 16);
    }
}

// ---------------------------------------------------------------------------
// Window plans (rows; the same receptive-field arithmetic as the f32 plans).
// Diagnostic build only (-DM2_STAMPS): per-wave s_memtime stamps at phase
// boundaries, [kernel][workgroup][wave][16] (tools/probe/stamps.py --x3).
#ifdef M2_STAMPS
__device__ unsigned long long g_x3_stamps[3][4096][16][16];
#define XSTAMP(K, i)                                                                                     \
    do {                                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                               \
        unsigned long long _t;                                                                           \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");                      \
        __builtin_amdgcn_sched_barrier(0);                                                               \
        const int _wg = blockIdx.y * gridDim.x + blockIdx.x;                                             \
        if ((threadIdx.x & 63) == 0 && _wg < 4096) g_x3_stamps[K][_wg][threadIdx.x >> 6][i] = _t;        \
    } while (0)
// s_memrealtime (100 MHz) into slot i: with an s_memtime pair of the same
// wave it gives the shader clock over that interval (tools/probe/stamps.py)
#define XSTAMP_RT(K, i)                                                                                  \
    do {                                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                               \
        unsigned long long _t;                                                                           \
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");                  \
        __builtin_amdgcn_sched_barrier(0);                                                               \
        const int _wg = blockIdx.y * gridDim.x + blockIdx.x;                                             \
        if ((threadIdx.x & 63) == 0 && _wg < 4096) g_x3_stamps[K][_wg][threadIdx.x >> 6][i] = _t;        \
    } while (0)
#else
#define XSTAMP(K, i) \
    do {             \
    } while (0)
#define XSTAMP_RT(K, i) \
    do {                \
    } while (0)
#endif

// COMP (stage1 planar head): input_conv composed into ConvT1
// (head_convT1c_planar; w.hc / w.hcb / w.hce).
template <class Cfg, bool TRANS, bool COMP = false>
__global__ __launch_bounds__(Cfg::HW * 64, Cfg::HMIN) void x3_head_kernel(const float* __restrict__ mel, int T,
                                                                            VocX w, unsigned char* __restrict__ U1,
                                                                            int items) {
    if (w.rclear && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 5) {
        if (threadIdx.x == 0) *reinterpret_cast<volatile int*>(w.rclear) = 0;
        else if (w.rqueue) reinterpret_cast<volatile unsigned*>(w.rqueue)[threadIdx.x - 1] = 0u;
    }
    if (w.head_prio == 1) {  // waves w, w + 4, ... share a SIMD; age favours the older ones
        const int pr = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) >> 2;
        if (pr == 1) __builtin_amdgcn_s_setprio(1);
        else if (pr == 2) __builtin_amdgcn_s_setprio(2);
        else if (pr >= 3) __builtin_amdgcn_s_setprio(3);
    }
    constexpr int M = Cfg::M, MP = Cfg::MP, C = Cfg::C, TF = Cfg::TF;
    const int wx = blockIdx.x, wy = blockIdx.y;
    if (w.dT) {  // speculative launch: T was the capacity
        T = dev_frames(w.dT, T);
        if (wx * TF >= T) return;
    }
    using Pl = HeadPlan<MP, C, TF, head_planar<Cfg>()>;
    constexpr int C1 = Pl::C1;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int b = wy, f0 = wx * TF;
    XW a0w{lds, f0 - 2};
    XW hw{lds, 4 * f0 - 1};
    XW melw{lds + Pl::RA, f0 - 3};
    XW uw{lds + Pl::RA, 4 * f0 - 4};
    constexpr int NW = Cfg::HW;
    using I0 = Conv3Items<MP, C, Cfg::NT_IN, Pl::A0_N, 1>;
    using I1 = ConvTItems<C, C1, 4, Cfg::NT_T1, Pl::NQ, 1>;
    using I2 = Conv3Items<C1, C1, Cfg::NT_R1, Pl::H_N, 1>;
    using I3 = Conv3Items<C1, C1, Cfg::NT_R1, Pl::O_N, 1>;
    // One item per wave in every layer (stage1): weight fragments handed
    // from layer to layer across the barriers (APipe).
    constexpr bool ONE = I0::N == NW && I1::N == NW && I2::N == NW &&
                         I3::N == NW && pd_of<MP, 3, 1>() == 4 && pd_of<C, 2, 1>() == 4 && pd_of<C1, 3, 1>() == 4;
    // phase-planar ConvT1 / ResBlock1: planes of 64 rows hold TF + 2 <= 65
    // input columns, one item per wave = (phase, m-block)
    constexpr bool PLANAR = ONE && head_planar<Cfg>();
    XSTAMP_RT(0, 14);
    XSTAMP(0, 0);
    if constexpr (COMP && !PLANAR) {
        // stage2: the composed layer on the generic item path; the mel window
        // in region A (the u rows it feeds are region B), edge terms after it
        static_assert(!ONE, "generic path");
        static_assert(Pl::CAP_MEL * Pl::RS_M + 4 * 4 * C1 <= Pl::RA, "mel window + edge terms in region A");
        static_assert(4 * C1 <= Cfg::HW * 64, "one thread per edge term");
        const XW melA{lds, f0 - 3};
        unsigned char* corr = lds + Pl::CAP_MEL * Pl::RS_M;
        // ConvT1's input columns here are [f0 - 1, f0 + TF]
        const bool left = f0 == 0, right = T - 1 >= f0 - 1 && T - 1 <= f0 + TF;
        gload_mel<TRANS, M, MP, Pl::RS_M, Pl::MEL_N, Cfg::HW * 64>(mel + (size_t)b * M * T, T, melA);
        XSTAMP(0, 1);
        __syncthreads();
        if (left || right) {
            head_edge_terms_s2<M, MP, C1, Pl::RS_M>(w.hce, melA, T, left, right, corr);
            __syncthreads();
        }
        XSTAMP(0, 2);
        XSTAMP(0, 3);
        XSTAMP(0, 4);
        xconvT1c<MP, C1, Cfg::NT_T1, Pl::RS_M, Pl::RS_1, Pl::NQ, Cfg::PDM, Cfg::HBP>(w.hc, w.hcb, (left || right) ? corr : nullptr, melA,
                                                              uw, f0 - 1, T);
        XSTAMP(0, 5);
        __syncthreads();
        XSTAMP(0, 6);
        xconv3<C1, C1, Cfg::NT_R1, ACT_LEAKY, false, Pl::RS_1, Pl::RS_1, Pl::H_N, 1, 0, false, Cfg::PDM, Cfg::HBP>(w.w1[0], w.b1[0], uw, hw, 4 * f0 - 1,
                                                                                 4 * T);
        XSTAMP(0, 7);
        __syncthreads();
        XSTAMP(0, 8);
        xconv3<C1, C1, Cfg::NT_R1, ACT_NONE, true, Pl::RS_1, Pl::RS_1, Pl::O_N, 1, 0, true, Cfg::PDM, Cfg::HBP>(
            w.w2[0], w.b2[0], hw, uw, 4 * f0, 4 * T, nullptr, nullptr, U1 + (size_t)b * 4 * T * 4 * C1);
        XSTAMP(0, 9);
        return;
    } else if constexpr (COMP) {
        static_assert(PLANAR, "the composed head runs on the phase-planar path");
        const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        constexpr int MB1 = C1 / 16;
        APipe ap;
        const u32x4* wp0 = w.hc + (size_t)wv * nkb_of<MP, 4>() * 128 + (threadIdx.x & 63);
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            ap[kb][0][0] = wp0[kb * 128];
            ap[kb][0][1] = wp0[kb * 128 + 64];
        }
        // the mel window goes to region A (the u planes it feeds are written
        // into region B in the same phase; the h planes overwrite it later)
        static_assert(Pl::CAP_MEL * Pl::RS_M + 4 * 4 * C1 <= Pl::RA, "mel window + edge terms in region A");
        const XW melA{lds, f0 - 3};
        unsigned char* corr = lds + Pl::CAP_MEL * Pl::RS_M;
        // the windows holding an utterance edge (workgroup-uniform)
        const bool left = f0 == 0, right = T - 1 >= f0 - 1 && T - 1 < f0 + TF;
        float4 ev[4];
        float eb = 0.f;
        if (left || right) head_edge_load<MP, C1>(w.hce, ev, eb);
        gload_mel<TRANS, M, MP, Pl::RS_M, Pl::MEL_N, Cfg::HW * 64>(mel + (size_t)b * M * T, T, melA);
        XSTAMP(0, 1);
        __syncthreads();
        if (left || right) {
            head_edge_terms<MP, C1, Pl::RS_M>(ev, eb, melA, T, left, right, corr);
            __syncthreads();
        }
        XSTAMP(0, 2);
        XSTAMP(0, 3);  // (no input-conv layer)
        XSTAMP(0, 4);
        unsigned char* up = lds + Pl::RA;
        unsigned char* hp = lds;
        head_convT1c_planar<MP, C1, Pl::RS_M, Pl::RS_1>(
            w.hc, w.hcb, (left || right) ? corr : nullptr, melA, up, f0, T, &ap,
            w.w1[0] + (size_t)rb1_mb<MB1>(wv, items) * nkb_of<C1, 3>() * 128 + (threadIdx.x & 63));
        XSTAMP(0, 5);
        __syncthreads();
        XSTAMP(0, 6);
        head_rb1_planar<C1, Pl::RS_1, false>(w.w1[0], w.b1[0], up, hp, nullptr, f0, TF, 4 * T, &ap,
                                             w.w2[0] + (size_t)rb1_mb<MB1>(wv, items) * nkb_of<C1, 3>() * 128 +
                                                 (threadIdx.x & 63),
                                             nullptr, 0, items);
        XSTAMP(0, 7);
        __syncthreads();
        XSTAMP(0, 8);
        head_rb1_planar<C1, Pl::RS_1, true>(w.w2[0], w.b2[0], hp, nullptr, up, f0, TF, 4 * T, &ap, nullptr,
                                            U1 + (size_t)b * 4 * T * 4 * C1, 0, items);
        XSTAMP(0, 9);
        XSTAMP_RT(0, 15);
        return;
    } else if constexpr (ONE) {
        const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        APipe ap;
        const u32x4* wp0 = I0::wp(w.wi, wv);
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            ap[kb][0][0] = wp0[kb * 128];
            ap[kb][0][1] = wp0[kb * 128 + 64];
        }
        gload_mel<TRANS, M, MP, Pl::RS_M, Pl::MEL_N, Cfg::HW * 64>(mel + (size_t)b * M * T, T, melw);
        XSTAMP(0, 1);
        __syncthreads();
        XSTAMP(0, 2);
        static_assert(PLANAR, "one item per wave: the phase-planar head");
        // phase-planar ConvT1 / ResBlock1 (u planes in region B, h planes in region A)
        unsigned char* up = lds + Pl::RA;
        unsigned char* hp = lds;
        xconv3<MP, C, Cfg::NT_IN, ACT_NONE, false, Pl::RS_M, Pl::RS_C, Pl::A0_N, 1, NW>(
            w.wi, w.bi, melw, a0w, f0 - 2, T, &ap, w.wt[0] + (size_t)wv * nkb_of<C, 2>() * 128 + (threadIdx.x & 63));
        XSTAMP(0, 3);
        __syncthreads();
        XSTAMP(0, 4);
        constexpr int MB1 = C1 / 16;
        head_convT1_planar<C, C1, Pl::RS_C, Pl::RS_1>(w.wt[0], w.bt[0], a0w, up, f0, 4 * T, &ap,
                                                    w.w1[0] + (size_t)rb1_mb<MB1>(wv, items) * nkb_of<C1, 3>() * 128 +
                                                        (threadIdx.x & 63));
        XSTAMP(0, 5);
        __syncthreads();
        XSTAMP(0, 6);
        head_rb1_planar<C1, Pl::RS_1, false>(w.w1[0], w.b1[0], up, hp, nullptr, f0, TF, 4 * T, &ap,
                                             w.w2[0] + (size_t)rb1_mb<MB1>(wv, items) * nkb_of<C1, 3>() * 128 +
                                                 (threadIdx.x & 63),
                                             nullptr, 0, items);
        XSTAMP(0, 7);
        __syncthreads();
        XSTAMP(0, 8);
        head_rb1_planar<C1, Pl::RS_1, true>(w.w2[0], w.b2[0], hp, nullptr, up, f0, TF, 4 * T, &ap, nullptr,
                                            U1 + (size_t)b * 4 * T * 4 * C1, 0, items);
        XSTAMP(0, 9);
        XSTAMP_RT(0, 15);
        return;
    } else {
        gload_mel<TRANS, M, MP, Pl::RS_M, Pl::MEL_N, Cfg::HW * 64>(mel + (size_t)b * M * T, T, melw);
        XSTAMP(0, 1);
        __syncthreads();
        XSTAMP(0, 2);
        xconv3<MP, C, Cfg::NT_IN, ACT_NONE, false, Pl::RS_M, Pl::RS_C, Pl::A0_N>(w.wi, w.bi, melw, a0w, f0 - 2, T);
        XSTAMP(0, 3);
        __syncthreads();
        XSTAMP(0, 4);
        xconvT<C, C1, 4, Cfg::NT_T1, Pl::RS_C, Pl::RS_1, Pl::NQ>(w.wt[0], w.bt[0], a0w, uw, f0 - 1, 4 * T);
        XSTAMP(0, 5);
        __syncthreads();
        XSTAMP(0, 6);
        xconv3<C1, C1, Cfg::NT_R1, ACT_LEAKY, false, Pl::RS_1, Pl::RS_1, Pl::H_N>(w.w1[0], w.b1[0], uw, hw, 4 * f0 - 1,
                                                                                 4 * T);
        XSTAMP(0, 7);
        __syncthreads();
        XSTAMP(0, 8);
        xconv3<C1, C1, Cfg::NT_R1, ACT_NONE, true, Pl::RS_1, Pl::RS_1, Pl::O_N>(w.w2[0], w.b2[0], hw, uw, 4 * f0, 4 * T);
    }
    XSTAMP(0, 9);
    __syncthreads();
    XSTAMP(0, 10);
    gstore_rows<C1, Pl::RS_1, Pl::O_N, Cfg::HW * 64>(U1 + (size_t)b * 4 * T * 4 * C1, 4 * T, uw, 4 * f0);
    XSTAMP(0, 11);
}

// ---------------------------------------------------------------------------
// headmid_kernel (stage1): the composed planar head and the pipelined mid
// stage (vocoder_midp.h) in one launch, U1 handed over in LDS.
//
// The mid's true dependency on U1 is +-1 column, and the head's planes give
// 4 TF = 252 valid U1 positions (256 u positions less two k3 convs), so a
// workgroup owns a strip of S <= 250 columns [qa, qa + S) and its window is
// the 252 positions from qa - 1.  qa - 1 is no multiple of 4 in general: the
// window starts at 4 f0 + rot and the head's planes are rotated by rot
// (head_convT1c_planar).  ResBlock1's conv2 writes U1 back into the u planes
// (0 outside the utterance, which is what the mid's loader delivers for such
// columns); after one barrier region A - the mel window, then the h planes -
// is dead and holds the mid's rings R1 and R2, and the mid's layer 0 reads the
// planes where midp_kernel reads ring R0.  No loader wave, no U1 in global
// memory, one launch boundary less.  Every output keeps its operation
// sequence: U2 is bit-identical to the two launches'.
// The mid's roles take 12 of the 16 waves; the others only keep the step
// barriers.  A role's first four k-blocks of weight fragments (8 of its 12 -
// 16 KB) are handed over like the head's from layer to layer: ResBlock1's
// conv2 issues their loads after its last MFMA, so they fly across its
// epilogue and the barrier; the role fetches the rest when it starts
// (-DM2_ROLE_PREFETCH=0, an A/B build: all of them then, as in midp_kernel).
#ifndef M2_ROLE_PREFETCH
#define M2_ROLE_PREFETCH 1
#endif
struct HmPlan {
    using Pl = HeadPlan<CfgS1::MP, CfgS1::C, CfgS1::TF, true>;
    static constexpr int S_MAX = kHeadmidSMax;  // owned columns + one on either side = the valid positions
    static_assert(Pl::LDS_BYTES == kHeadmidLds, "the plan's LDS bytes");
    struct Lay {
        static constexpr bool PLANES = true;
        static constexpr int R0_OFF = 0, R1_OFF = 0, R2_OFF = mp::RROWS * mp::RS1;  // (no R0)
        static constexpr int U_OFF = Pl::RA;
    };
    static constexpr int NCH_MAX = (S_MAX + 15) / 16;
    static_assert(head_planar<CfgS1>() && CfgS1::HW == 16, "the phase-planar head of 16 waves");
    static_assert(Pl::RS_1 == mp::PRS && kPlane == mp::PROWS, "layer 0 of the mid reads the head's u planes");
    static_assert(Lay::R2_OFF + mp::RROWS * mp::RS1 <= Pl::RA, "rings R1 and R2 in region A");
    // layer 0 reads window positions -14 .. 16 NCH_MAX + 3: rows -4 .. 4 NCH_MAX + 1 of a plane
    static_assert(Lay::U_OFF >= 4 * mp::PRS, "the warm-up chunk's rows stay inside LDS");
    static_assert(Lay::U_OFF + (3 * mp::PROWS + 4 * NCH_MAX + 2) * mp::PRS <= Pl::LDS_BYTES,
                  "the last chunk's rows stay inside LDS");
};

template <bool TRANS, int NCHC>
__global__ __launch_bounds__(CfgS1::HW * 64, CfgS1::HMIN) void headmid_kernel(const float* __restrict__ mel, int T,
                                                                               VocX w, unsigned char* __restrict__ U2,
                                                                               int S, int nch_arg, int items) {
    if (w.rclear && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 5) {
        if (threadIdx.x == 0) *reinterpret_cast<volatile int*>(w.rclear) = 0;
        else if (w.rqueue) reinterpret_cast<volatile unsigned*>(w.rqueue)[threadIdx.x - 1] = 0u;
    }
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w.head_prio == 1) {
        const int pr = wv >> 2;
        if (pr == 1) __builtin_amdgcn_s_setprio(1);
        else if (pr == 2) __builtin_amdgcn_s_setprio(2);
        else if (pr >= 3) __builtin_amdgcn_s_setprio(3);
    }
    using Cfg = CfgS1;
    using Pl = HmPlan::Pl;
    using Lay = HmPlan::Lay;
    constexpr int M = Cfg::M, MP = Cfg::MP, TF = Cfg::TF, C1 = Pl::C1, MB1 = C1 / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int nch = NCHC ? NCHC : nch_arg;
    const int b = blockIdx.y, qa = blockIdx.x * S, L1 = 4 * T;
    const int o = qa - 1, f0 = o >> 2, rot = o & 3;  // the window: positions [4 f0 + rot, + 252)
    APipe ap;
    {
        const int it0 = (((wv / MB1) + rot) & 3) * MB1 + wv % MB1;  // this wave's ConvT1 item: (phase, m-block)
        const u32x4* wp0 = w.hc + (size_t)it0 * nkb_of<MP, 4>() * 128 + (threadIdx.x & 63);
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            ap[kb][0][0] = wp0[kb * 128];
            ap[kb][0][1] = wp0[kb * 128 + 64];
        }
    }
    static_assert(Pl::CAP_MEL * Pl::RS_M + 4 * 4 * C1 <= Pl::RA, "mel window + edge terms in region A");
    const XW melA{lds, f0 - 3};
    unsigned char* corr = lds + Pl::CAP_MEL * Pl::RS_M;
    // the windows whose planes hold input column 0 / T - 1 (columns f0 - 1 .. f0 + 64 at the most)
    const bool left = f0 <= 1, right = T - 1 >= f0 - 1 && T - 1 <= f0 + 64;
    float4 ev[4];
    float eb = 0.f;
    if (left || right) head_edge_load<MP, C1>(w.hce, ev, eb);
    gload_mel<TRANS, M, MP, Pl::RS_M, Pl::MEL_N, Cfg::HW * 64>(mel + (size_t)b * M * T, T, melA);
    __syncthreads();
    if (left || right) {
        head_edge_terms<MP, C1, Pl::RS_M>(ev, eb, melA, T, left, right, corr);
        __syncthreads();
    }
    unsigned char* up = lds + Pl::RA;
    unsigned char* hp = lds;
    const u32x4* wr1 = w.w1[0] + (size_t)rb1_mb<MB1>(wv, items) * nkb_of<C1, 3>() * 128 + (threadIdx.x & 63);
    const u32x4* wr2 = w.w2[0] + (size_t)rb1_mb<MB1>(wv, items) * nkb_of<C1, 3>() * 128 + (threadIdx.x & 63);
    head_convT1c_planar<MP, C1, Pl::RS_M, Pl::RS_1>(w.hc, w.hcb, (left || right) ? corr : nullptr, melA, up, f0, T,
                                                    &ap, wr1, rot);
    __syncthreads();
    head_rb1_planar<C1, Pl::RS_1, false>(w.w1[0], w.b1[0], up, hp, nullptr, f0, TF, L1, &ap, wr2, nullptr, rot,
                                         items);
    __syncthreads();
    constexpr bool PREF = M2_ROLE_PREFETCH != 0;
    static_assert(sizeof(APipe) == mp::kPre * 2 * sizeof(u32x4), "the hand-over holds the roles' first k-blocks");
    head_rb1_planar<C1, Pl::RS_1, true, true>(w.w2[0], w.b2[0], hp, nullptr, up, f0, TF, L1, &ap,
                                              PREF && wv < 12 ? mp::role_wp(w.mp, wv) : nullptr, nullptr, rot, items);
    __syncthreads();  // U1 of the window is in the u planes; region A is dead
    // the mid's pipeline over the strip (midp_kernel's roles and step protocol)
    const bool edge = qa < 16 || qa + 16 * nch + 16 > L1;
    const int xown = min(L1, qa + S);
    unsigned char* u2row = U2 + (size_t)b * 4 * L1 * 128;
    const u32x4* W = w.mp;
    const float* bias = w.mpb;
    const int layer = wv < 12 ? wv >> 2 : 3;
    if (layer == 2) __builtin_amdgcn_s_setprio(2);  // later layers: younger waves, the step waits for them
    else if (layer == 1) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
    switch (wv) {
        case 0: mp::layer_role<0, 0, Lay, 0, 2, PREF>(lds, qa, L1, nch, edge, W, bias, u2row, xown, ap); break;
        case 1: mp::layer_role<0, 1, Lay, 0, 2, PREF>(lds, qa, L1, nch, edge, W, bias, u2row, xown, ap); break;
        case 2: mp::layer_role<0, 2, Lay, 0, 2, PREF>(lds, qa, L1, nch, edge, W, bias, u2row, xown, ap); break;
        case 3: mp::layer_role<0, 3, Lay, 0, 2, PREF>(lds, qa, L1, nch, edge, W, bias, u2row, xown, ap); break;
        case 4: mp::layer_role<1, 0, Lay, 0, 2, PREF>(lds, qa, L1, nch, edge, W, bias, u2row, xown, ap); break;
        case 5: mp::layer_role<1, 1, Lay, 0, 2, PREF>(lds, qa, L1, nch, edge, W, bias, u2row, xown, ap); break;
        case 6: mp::layer_role<1, 2, Lay, 0, 2, PREF>(lds, qa, L1, nch, edge, W, bias, u2row, xown, ap); break;
        case 7: mp::layer_role<1, 3, Lay, 0, 2, PREF>(lds, qa, L1, nch, edge, W, bias, u2row, xown, ap); break;
        case 8: mp::layer_role<2, 0, Lay, 0, 2, PREF>(lds, qa, L1, nch, edge, W, bias, u2row, xown, ap); break;
        case 9: mp::layer_role<2, 1, Lay, 0, 2, PREF>(lds, qa, L1, nch, edge, W, bias, u2row, xown, ap); break;
        case 10: mp::layer_role<2, 2, Lay, 0, 2, PREF>(lds, qa, L1, nch, edge, W, bias, u2row, xown, ap); break;
        case 11: mp::layer_role<2, 3, Lay, 0, 2, PREF>(lds, qa, L1, nch, edge, W, bias, u2row, xown, ap); break;
        default:  // no role: the step barriers only
#pragma unroll 1
            for (int s = -1; s <= nch + 2; ++s) pipe::step_barrier();
            break;
    }
}

std::atomic<long> g_headmid_launches{0};

template <class Cfg>
__global__ __launch_bounds__(Cfg::MW * 64, Cfg::MMIN) void x3_mid_kernel(const unsigned char* __restrict__ U1,
                                                                           int L1, VocX w,
                                                                           unsigned char* __restrict__ U2) {
    constexpr int CI = Cfg::C / 2, W = Cfg::W2;
    using Pl = MidPlan<CI, W>;
    constexpr int CO = Pl::CO;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int b = blockIdx.y, p0 = blockIdx.x * W;
    if (w.dT) {  // speculative launch: L1 was the capacity
        L1 = 4 * dev_frames(w.dT, L1 / 4);
        if (p0 >= L1) return;
    }
    const int L2 = 4 * L1;
    XW inw{lds, p0 - 2};
    XW hw{lds, 4 * p0 - 1};
    XW uw{lds + Pl::RA, 4 * p0 - 4};
    XSTAMP(1, 0);
    gload_rows<CI, Pl::RS_I, Pl::IN_N, Cfg::MW * 64>(U1 + (size_t)b * L1 * 4 * CI, L1, inw);
    XSTAMP(1, 1);
    __syncthreads();
    XSTAMP(1, 2);
    xconvT<CI, CO, 4, Cfg::NT_T2, Pl::RS_I, Pl::RS_O, Pl::NQ, 1, 0, Cfg::PDM>(w.wt[1], w.bt[1], inw, uw, p0 - 1, L2);
    XSTAMP(1, 3);
    __syncthreads();
    XSTAMP(1, 4);
    xconv3<CO, CO, Cfg::NT_R2, ACT_LEAKY, false, Pl::RS_O, Pl::RS_O, Pl::H_N, 1, 0, false, Cfg::PDM>(w.w1[1], w.b1[1], uw, hw, 4 * p0 - 1, L2);
    XSTAMP(1, 5);
    __syncthreads();
    XSTAMP(1, 6);
    xconv3<CO, CO, Cfg::NT_R2, ACT_NONE, true, Pl::RS_O, Pl::RS_O, Pl::O_N, 1, 0, false, Cfg::PDM>(w.w2[1], w.b2[1], hw, uw, 4 * p0, L2);
    XSTAMP(1, 7);
    __syncthreads();
    XSTAMP(1, 8);
    gstore_rows<CO, Pl::RS_O, Pl::O_N, Cfg::MW * 64>(U2 + (size_t)b * L2 * 4 * CO, L2, uw, 4 * p0);
    XSTAMP(1, 9);
}

template <class Cfg>
__global__ __launch_bounds__(Cfg::TW * 64, Cfg::TMIN) void x3_tail_kernel(const unsigned char* __restrict__ U2,
                                                                            int L2, VocX w,
                                                                            float* __restrict__ audio) {
    constexpr int CI = Cfg::C / 4, W = Cfg::W3;
    using Pl = TailPlan<CI, W>;
    constexpr int C3 = Pl::C3, C4 = Pl::C4;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int b = blockIdx.y, p0 = blockIdx.x * W;
    if (w.dT) {  // speculative launch: L2 was the capacity
        L2 = 16 * dev_frames(w.dT, L2 / 16);
        if (p0 >= L2) return;
    }
    const int L3 = 2 * L2, L4 = 4 * L2;
    unsigned char* ra = lds;
    unsigned char* rb = lds + Pl::RA;
    XW inw{ra, p0 - 4};
    XW u3{rb, 2 * p0 - 6};
    XW h3{ra, 2 * p0 - 4};
    XW u4{ra, 4 * p0 - 4};
    XW h4w{rb, 4 * p0 - 2};
    XSTAMP(2, 0);
    gload_rows<CI, Pl::RS_I, Pl::IN_N, Cfg::TW * 64>(U2 + (size_t)b * L2 * 4 * CI, L2, inw);
    XSTAMP(2, 1);
    __syncthreads();
    XSTAMP(2, 2);
    xconvT<CI, C3, 2, Cfg::NT_T3, Pl::RS_I, Pl::RS_3, Pl::NQ3, 1, 0, Cfg::PDM>(w.wt[2], w.bt[2], inw, u3, p0 - 3, L3);
    XSTAMP(2, 3);
    __syncthreads();
    XSTAMP(2, 4);
    xconv3<C3, C3, Cfg::NT_R3, ACT_LEAKY, false, Pl::RS_3, Pl::RS_3, Pl::H3_N, 1, 0, false, Cfg::PDM>(w.w1[2], w.b1[2], u3, h3, 2 * p0 - 4, L3);
    XSTAMP(2, 5);
    __syncthreads();
    XSTAMP(2, 6);
    xconv3<C3, C3, Cfg::NT_R3, ACT_NONE, true, Pl::RS_3, Pl::RS_3, Pl::O3_N, 1, 0, false, Cfg::PDM>(w.w2[2], w.b2[2], h3, u3, 2 * p0 - 3, L3);
    XSTAMP(2, 7);
    __syncthreads();
    XSTAMP(2, 8);
    xconvT<C3, C4, 2, Cfg::NT_T4, Pl::RS_3, Pl::RS_4, Pl::NQ4, 1, 0, Cfg::PDM>(w.wt[3], w.bt[3], u3, u4, 2 * p0 - 2, L4);
    XSTAMP(2, 9);
    __syncthreads();
    XSTAMP(2, 10);
    xconv3<C4, C4, Cfg::NT_R4, ACT_LEAKY, false, Pl::RS_4, Pl::RS_4, Pl::H4_N, 1, 0, false, Cfg::PDM>(w.w1[3], w.b1[3], u4, h4w, 4 * p0 - 2, L4);
    XSTAMP(2, 11);
    __syncthreads();
    XSTAMP(2, 12);
    xconv3<C4, C4, Cfg::NT_R4, ACT_NONE, true, Pl::RS_4, Pl::RS_4, Pl::O4_N, 1, 0, false, Cfg::PDM>(w.w2[3], w.b2[3], h4w, u4, 4 * p0 - 1, L4);
    XSTAMP(2, 13);
    __syncthreads();
    XSTAMP(2, 14);
    // output_conv (C4 -> 1, k3) + tanh on the VALU, one sample per thread.
    float* arow = audio + (size_t)b * L4;
    const float bo = w.bo[0];
    for (int j = threadIdx.x; j < Pl::A_N; j += blockDim.x) {
        const int t = 4 * p0 + j;
        if (t < L4) {
            const unsigned char* x = u4.p + (t - 1 - u4.start) * Pl::RS_4;
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const _Float16* hr = reinterpret_cast<const _Float16*>(x + k * Pl::RS_4);
#pragma unroll
                for (int ci = 0; ci < C4; ++ci)
                    acc = fmaf(w.wo[ci * 3 + k], (float)hr[ci] + (float)hr[C4 + ci], acc);
            }
            const float o = tanhf(acc + bo);
            arow[t] = o;
            flag_nonfinite4(o, 0.f, 0.f, 0.f, w.rflag);
        }
    }
    XSTAMP(2, 15);
}

// One row per kernel instantiation (KernelRow, vocoder_fused.h): the row serves
// the LDS attribute, the occupancy query and the launch.  Heads by
// [VocHead][comp][trans] (the 19 / 24 / 27-frame stage2 heads exist composed
// only: their other rows stay empty), mids and tails by [stage1, stage2,
// stage2 alt], headmid by [nch == 16][trans].
struct Rows {
    KernelRow head[5][2][2], mid[3], tail[3], headmid[2][2];
};
// r[trans] of a head / headmid variant
template <class Cfg, bool COMP>
void head_rows(KernelRow (&r)[2]) {
    r[0] = {reinterpret_cast<const void*>(&x3_head_kernel<Cfg, false, COMP>), Cfg::HW * 64, HeadPlanOf<Cfg>::LDS_BYTES};
    r[1] = {reinterpret_cast<const void*>(&x3_head_kernel<Cfg, true, COMP>), Cfg::HW * 64, HeadPlanOf<Cfg>::LDS_BYTES};
}
template <int NCHC>
void headmid_rows(KernelRow (&r)[2]) {
    r[0] = {reinterpret_cast<const void*>(&headmid_kernel<false, NCHC>), CfgS1::HW * 64, kHeadmidLds};
    r[1] = {reinterpret_cast<const void*>(&headmid_kernel<true, NCHC>), CfgS1::HW * 64, kHeadmidLds};
}
template <class Cfg>
KernelRow mid_row() {
    return {reinterpret_cast<const void*>(&x3_mid_kernel<Cfg>), Cfg::MW * 64, MidPlan<Cfg::C / 2, Cfg::W2>::LDS_BYTES};
}
template <class Cfg>
KernelRow tail_row() {
    return {reinterpret_cast<const void*>(&x3_tail_kernel<Cfg>), Cfg::TW * 64, TailPlan<Cfg::C / 4, Cfg::W3>::LDS_BYTES};
}
// (Filled in the order the kernels have always been instantiated in, which is
// the order of the device code in the object.)
Rows make_rows() {
    Rows r;
    head_rows<CfgS1, false>(r.head[(int)VocHead::S1][0]);
    head_rows<CfgS1, true>(r.head[(int)VocHead::S1][1]);
    r.mid[0] = mid_row<CfgS1>();
    r.tail[0] = tail_row<CfgS1>();
    headmid_rows<16>(r.headmid[1]);
    headmid_rows<0>(r.headmid[0]);
    r.tail[2] = tail_row<CfgS2Alt>();
    r.mid[2] = mid_row<CfgS2Alt>();
    head_rows<CfgS2, false>(r.head[(int)VocHead::S2T16][0]);
    head_rows<CfgS2, true>(r.head[(int)VocHead::S2T16][1]);
    r.mid[1] = mid_row<CfgS2>();
    r.tail[1] = tail_row<CfgS2>();
    head_rows<CfgS2H24, true>(r.head[(int)VocHead::S2H24][1]);
    head_rows<CfgS2T19, true>(r.head[(int)VocHead::S2T19][1]);
    head_rows<CfgS2H27, true>(r.head[(int)VocHead::S2H27][1]);
    return r;
}
const Rows kRows = make_rows();

// The one-time setup: every row's LDS attribute, then the workgroup slots the
// plan's rules weigh.  Thread-safe (a function-local static); a failed
// hipFuncSetAttribute stays the answer of every later call.
struct Setup {
    hipError_t err;
    VocSlots slots;
};
const Setup& setup() {
    static const Setup s = [] {
        Setup r;
        r.err = set_rows_lds(reinterpret_cast<const KernelRow*>(&kRows), sizeof(Rows) / sizeof(KernelRow));
        auto head = [](VocHead h) { return row_slots(kRows.head[(int)h][1][0]); };  // composed, [B, M, T]
        r.slots = {head(VocHead::S2T16), head(VocHead::S2T19), head(VocHead::S2H24), head(VocHead::S2H27),
                   row_slots(kRows.mid[1]), row_slots(kRows.mid[2]), row_slots(kRows.tail[1]), row_slots(kRows.tail[2])};
        return r;
    }();
    return s;
}

// Launches what the plan names (plan_vocoder_launch, vocoder_launch.h).
int32_t run(const float* mel, int T, const VocLaunchPlan& p, const VocX& w, void* U1, void* U2, float* audio,
            hipStream_t st, const std::function<void(int, bool)>& mark) {
    if (setup().err != hipSuccess) return hip_status(setup().err, "x3 vocoder: hipFuncSetAttribute (one-time setup)");
    int32_t rc;
    int L1 = 4 * T, L2 = 16 * T;
    VocX wv = w;
    int items = sw().head_items;  // ResBlock1's item map of the 16-wave planar head (head_rb1_planar)
    if (p.headmid) {
        void* args[] = {&mel, &T, &wv, &U2, const_cast<int*>(&p.hm_S), const_cast<int*>(&p.hm_nch), &items};
        if ((rc = launch_row(kRows.headmid[p.hm_nch == 16][p.trans], p.head_g, st, args, "headmid_kernel"))) return rc;
        g_headmid_launches.fetch_add(1, std::memory_order_relaxed);
    } else {
        mark(0, true);
        void* hargs[] = {&mel, &T, &wv, &U1, &items};
        rc = launch_row(kRows.head[(int)p.head][p.comp][p.trans], p.head_g, st, hargs, "x3_head_kernel");
        mark(0, false);
        if (rc) return rc;
        mark(1, true);
        if (p.mid == VocMid::Midp) {  // stage1: the pipelined mid stage (vocoder_midp.hip)
            rc = launch_vocoder_midp(U1, L1, p.mid_nch, p.mid_g, w.mp, w.mpb, U2, st, w.dT);
        } else {
            void* margs[] = {&U1, &L1, &wv, &U2};
            rc = launch_row(kRows.mid[p.mid == VocMid::X3Alt ? 2 : p.stage == 2], p.mid_g, st, margs,
                            "x3_mid_kernel");
        }
        if (rc) return rc;
        mark(1, false);
    }
    mark(2, true);
    if (p.tail == VocTail::Tailp2)  // stage2: the pipelined tail (vocoder_tailp2.hip)
        rc = launch_vocoder_tailp2(U2, L2, p.tail_nl, p.tail_nch, p.tail_g, w.tp2, w.tp2b, audio, w.rflag, st, w.dT,
                                   VocRedo{w.redo_w, mel, p.trans});
    else if (p.tail == VocTail::Tailp)  // stage1: the pipelined tail (vocoder_tailp.hip)
        rc = launch_vocoder_tailp(U2, L2, p.tail_nl, p.tail_nch, p.tail_g, w.tp, w.tpb, audio, w.rflag, st, w.dT,
                                  VocRedo{w.redo_w, mel, p.trans});
    else {
        void* targs[] = {&U2, &L2, &wv, &audio};
        rc = launch_row(kRows.tail[p.tail == VocTail::X3Alt ? 2 : p.stage == 2], p.tail_g, st, targs,
                        "x3_tail_kernel");
    }
    mark(2, false);
    return rc;
}

}  // namespace x3

const char* const kVocX3KernelNames[kVocKernels] = {
    "x3_head_kernel (input_conv + ConvT1 + ResBlock1)",
    "x3_mid_kernel (ConvT2 + ResBlock2)",
    "x3_tail_kernel (ConvT3 + ResBlock3 + ConvT4 + ResBlock4 + output_conv)"};

#ifdef M2_STAMPS
extern "C" int32_t m2_debug_stamps_x3(void* host, size_t bytes) {
    return (int32_t)hipMemcpyFromSymbol(host, HIP_SYMBOL(x3::g_x3_stamps),
                                        bytes < sizeof(x3::g_x3_stamps) ? bytes : sizeof(x3::g_x3_stamps));
}
#endif

extern "C" int64_t m2_debug_headmid_launches(void) { return x3::g_headmid_launches.load(std::memory_order_relaxed); }

bool vocoder_x3_supported(int M, int C) { return (M == 64 && C == 128) || (M == 80 && C == 256); }

int vocoder_x3_mel_pad(int M) { return M == 80 ? 96 : M; }

const VocSlots& vocoder_x3_slots() { return x3::setup().slots; }

extern "C" int32_t m2_debug_vocoder_slots(int64_t* out8) {
    if (!out8) return fail(M2_E_ARG, "m2_debug_vocoder_slots: null output");
    const VocSlots& s = vocoder_x3_slots();
    const long v[8] = {s.head16, s.head19, s.head24, s.head27, s.mid, s.mid_alt, s.tail, s.tail_alt};
    for (int i = 0; i < 8; ++i) out8[i] = v[i];
    return M2_OK;
}

int32_t launch_vocoder_x3(const float* mel, int T, const VocLaunchPlan& plan, const VocX& w, void* U1, void* U2,
                          float* audio, hipStream_t st, const std::function<void(int, bool)>& mark) {
    return x3::run(mel, T, plan, w, U1, U2, audio, st, mark);
}

// ---------------------------------------------------------------------------
// Host packing: [group = phase*MB + mb][kb][hi|lo][lane][8 halves] with
// A[co = mb*16 + (lane&15)][octet o = 4kb + (lane>>4), element e] =
// W(ph, co, ci = (o % NOCT)*8 + e, tap = o / NOCT); zero for co >= Cout or o >= NK.
namespace {
void put(std::vector<uint16_t>& out, size_t idx, float v, bool* range_ok) {
    if (!(std::fabs(v) < 65504.f)) *range_ok = false;
    const _Float16 h = (_Float16)v;
    const _Float16 l = (_Float16)(v - (float)h);
    uint16_t hb, lb;
    std::memcpy(&hb, &h, 2);
    std::memcpy(&lb, &l, 2);
    out[idx] = hb;
    out[idx + 64 * 8] = lb;
}

template <typename Wf>
std::vector<uint16_t> pack_x3(int NPH, int Cout, int Cin, int NTAP, Wf W, bool* range_ok) {
    const int MB = (Cout + 15) / 16, NOCT = Cin / 8, NK = NTAP * NOCT, NKB = (NK + 3) / 4;
    std::vector<uint16_t> out((size_t)NPH * MB * NKB * 2 * 64 * 8, 0);
    for (int ph = 0; ph < NPH; ++ph)
        for (int mb = 0; mb < MB; ++mb)
            for (int kb = 0; kb < NKB; ++kb)
                for (int lane = 0; lane < 64; ++lane) {
                    const int co = mb * 16 + (lane & 15), o = 4 * kb + (lane >> 4);
                    if (co >= Cout || o >= NK) continue;
                    const int tap = o / NOCT;
                    for (int e = 0; e < 8; ++e) {
                        const int ci = (o % NOCT) * 8 + e;
                        const size_t idx = ((((size_t)(ph * MB + mb) * NKB + kb) * 2) * 64 + lane) * 8 + e;
                        put(out, idx, W(ph, co, ci, tap), range_ok);
                    }
                }
    return out;
}
}  // namespace

std::vector<uint16_t> pack_x3_conv3(const float* W, int Cout, int Cin, int CinPad, bool* range_ok, bool res) {
    std::vector<uint16_t> out = pack_x3(
        1, Cout, CinPad, 3,
        [&](int, int co, int ci, int tap) { return ci < Cin ? W[((size_t)co * Cin + ci) * 3 + tap] : 0.f; }, range_ok);
    if (res && res_fold_channels(Cin)) {
        // Identity on the padding octets of the last k-block (x octet o - NK):
        // hi = 1.0 (0x3c00), lo = 0.
        const int NOCT = Cin / 8, NK = 3 * NOCT, NKB = (NK + 3) / 4, kb = NKB - 1;
        for (int lane = 0; lane < 64; ++lane) {
            const int co = lane & 15, o = 4 * kb + (lane >> 4);
            if (o < NK || co >= Cout) continue;
            for (int e = 0; e < 8; ++e)
                if ((o - NK) * 8 + e == co) out[(((size_t)kb * 2) * 64 + lane) * 8 + e] = 0x3c00;
        }
    }
    return out;
}

// input_conv o ConvT1 for the composed stage1 head (head_convT1c_planar), in
// double: Wc(ph, co, m, k) = sum_{j = 0, 1; tin = j + 2 - k in [0, 2]} sum_ci
// W_T[ci][co][kj(ph)] W_in[ci][m][tin] (ConvT tap j: input frame q + d0 - j,
// kernel index kj; input-conv tap tin: mel frame i - 1 + tin); bc[ph][co] =
// b_T[co] + sum_j sum_ci W_T[ci][co][kj] b_in[ci]; edge tables E[ph][co][m] =
// sum_ci W_T[ci][co][k_edge] W_in[ci][m][2 (ph < 2) | 0], e[ph][co] = sum_ci
// W_T[ci][co][k_edge] b_in[ci], k_edge = k1 (frame -1) for ph < 2, k0 (frame T).
bool pack_x3_head_comp(const float* Win, const float* bin, const float* WT, const float* bT, int M, int MP, int C,
                       std::vector<uint16_t>* w, std::vector<float>* bias, std::vector<float>* edge, bool* range_ok) {
    const int C1 = C / 2, R = 4, P = R / 2;
    if (MP % 8 || MP < M) return false;
    auto kj = [&](int ph, int j) {
        const int k0 = (ph + P < R) ? ph + P : ph + P - R, k1 = (ph + P < R) ? ph + P + R : ph + P;
        return j ? k1 : k0;
    };
    auto wt = [&](int ci, int co, int k) { return (double)WT[((size_t)ci * C1 + co) * 2 * R + k]; };
    auto wi = [&](int ci, int m, int k) { return m < M ? (double)Win[((size_t)ci * M + m) * 3 + k] : 0.0; };
    std::vector<double> wc((size_t)R * C1 * MP * 4, 0.0);  // [ph][co][m][k]
    for (int ph = 0; ph < R; ++ph)
        for (int co = 0; co < C1; ++co)
            for (int j = 0; j < 2; ++j) {
                const int k = kj(ph, j);
                for (int ci = 0; ci < C; ++ci) {
                    const double a = wt(ci, co, k);
                    for (int tin = 0; tin < 3; ++tin) {
                        const int kk = j + 2 - tin;  // composed tap: mel frame q + d0 + 1 - kk
                        for (int m = 0; m < M; ++m) wc[(((size_t)ph * C1 + co) * MP + m) * 4 + kk] += a * wi(ci, m, tin);
                    }
                }
            }
    *w = pack_x3(R, C1, MP, 4, [&](int ph, int co, int m, int k) { return (float)wc[(((size_t)ph * C1 + co) * MP + m) * 4 + k]; },
                 range_ok);
    bias->assign((size_t)R * C1, 0.f);
    edge->assign((size_t)R * C1 * MP + (size_t)R * C1, 0.f);
    for (int ph = 0; ph < R; ++ph)
        for (int co = 0; co < C1; ++co) {
            double b = bT[co];
            for (int j = 0; j < 2; ++j)
                for (int ci = 0; ci < C; ++ci) b += wt(ci, co, kj(ph, j)) * bin[ci];
            (*bias)[(size_t)ph * C1 + co] = (float)b;
            const int ke = kj(ph, ph < 2 ? 1 : 0), tin = ph < 2 ? 2 : 0;
            double e = 0.0;
            for (int ci = 0; ci < C; ++ci) e += wt(ci, co, ke) * bin[ci];
            (*edge)[(size_t)R * C1 * MP + (size_t)ph * C1 + co] = (float)e;
            for (int m = 0; m < M; ++m) {
                double v = 0.0;
                for (int ci = 0; ci < C; ++ci) v += wt(ci, co, ke) * wi(ci, m, tin);
                (*edge)[((size_t)ph * C1 + co) * MP + m] = (float)v;
            }
        }
    return true;
}

std::vector<uint16_t> pack_x3_convT(const float* W, int Cin, int Cout, int R, bool* range_ok) {
    const int P = R / 2;
    return pack_x3(R, Cout, Cin, 2,
                   [&](int ph, int co, int ci, int tap) {
                       const int k0 = (ph + P < R) ? ph + P : ph + P - R;  // tap 0: x[q] or x[q+1]
                       const int k1 = (ph + P < R) ? ph + P + R : ph + P;  // tap 1: x[q-1] or x[q]
                       return W[((size_t)ci * Cout + co) * 2 * R + (tap ? k1 : k0)];
                   },
                   range_ok);
}

}  // namespace m2
