// The layer role of the pipelined stage1 mid stage (ConvT2 + ResBlock2,
// vocoder_midp.hip), shared by midp_kernel and headmid_kernel (vocoder_x3.hip:
// the head and the mid in one launch).  The role is templated on where the
// rings sit in LDS and on where layer 0 reads its input: ring R0, filled by a
// loader wave from U1 in global memory, or the head's u planes, where
// ResBlock1 left U1 in place.
#pragma once
#include "m2_common.h"
#include "vocoder_fused.h"
#include "vocoder_pipe.h"

namespace m2 {
namespace mp {

using namespace pipe;  // vector types, mfma_h, step_barrier

// Cache policy of conv2's U2 stores (gstore16, m2_common.h; a build define
// for the A/B): write-through.  U2 (32.8 MB at B=32, T=500) is read by the
// next launch, mostly from another XCD; plain stores left it dirty in the
// writing XCD's L2 for the launch boundary to write back.  Write-through
// measured 3.4 us per call faster than plain at that shape (non-temporal
// 2.9), in every alternation pair (profiles/r15/r15_store_ab.txt).
#ifndef M2_U2_STORE
#define M2_U2_STORE 1
#endif

constexpr int RROWS = 64;               // 4 chunks of 16 columns
constexpr int RS0 = 288;                // R0 row: 256 B (hi[64] lo[64]) + pad, RS/16 = 2 mod 4
constexpr int RS1 = 544;                // R1/R2 row: 512 B (hi[128] lo[128]) + pad

// midp_kernel's LDS: the three rings one after the other.
struct RingLay {
    static constexpr bool PLANES = false;
    static constexpr int R0_OFF = 0, R1_OFF = RROWS * RS0, R2_OFF = R1_OFF + RROWS * RS1;
    static constexpr int U_OFF = 0;
    static constexpr int LDS_BYTES = R2_OFF + RROWS * RS1;
};

// The head's u planes as layer 0's input (vocoder_x3.hip, "Phase-planar
// head"): 4 planes of PROWS rows of PRS bytes from U_OFF, plane v holding
// window positions e = 4 i + v at row i + (v >= 2), 16-B chunks c and c ^ 1
// swapped in rows with bit 2 set.
constexpr int PROWS = 64, PRS = 288;

// Byte offset of 16-B unit u in row `row` of ring R1 / R2 (stride RS1): units
// swap pairwise (u ^ 1) in rows 4-7 of every 8.  With RS1 / 16 = 2 (mod 4) the
// B-fragment and residual reads (ds_read_b128, 16-lane groups) were already
// conflict-free but the epilogue stores (ds_write_b128: 8 consecutive rows,
// 32 banks) hit two-way conflicts; the swap makes all three conflict-free
// (tools/probe/midp_banks.py models every access of the kernel).
__device__ __forceinline__ unsigned r12_at(int row, int u) { return row * RS1 + 16 * (u ^ ((row >> 2) & 1)); }

// Layer L (0 ConvT2, 1 conv1, 2 conv2) of phase S: m-blocks 2S + HB ..
// 2S + HB + NH - 1 (both m-blocks of the phase by default).
// As in vocoder_tailp.hip: one fp32 accumulator per m-block for the three
// split products, LDS addresses precomputed for the four ring phases
// j = k mod 4 (step loop unrolled by four), leaky as a packed multiply and
// bare max, zeroing as a wave-uniform branch on chunks that straddle an
// utterance end, and conv2's residual (ConvT2's output, ring R1, two columns
// ahead: channels 32S .. 32S+31 = one fragment shared by both m-blocks) as
// two identity-A MFMAs per m-block instead of 24 VALU.
// Lay::PLANES (layer 0 only): the strip's window starts at column qa - 1, so
// the column qa + 2 + 16 k + li + dq that lane li reads in chunk k is window
// position e = 16 k + li + dq + 3: the plane and the row modulo 4 are fixed
// per lane, the row advances by 4 per chunk and its swizzle bit flips with
// the chunk's parity, which is the ring phase's (j = k mod 4 at layer 0).
// xown: conv2 stores the columns below it (the strip's owned columns end
// there, or the utterance does).
// PRE, pre (headmid_kernel): the role's first kPre k-blocks of weight fragments
// in the order the role holds them (its units are consecutive), whose loads
// the caller issued earlier from role_wp; the role fetches the rest.
// Else (midp_kernel): the role fetches all of them when it starts.
constexpr int kPre = 4;
// this lane's slot of the first unit of the role of wave wv (wv < 12: layer wv / 4, phase wv % 4)
__device__ __forceinline__ const u32x4* role_wp(const u32x4* __restrict__ W, int wv) {
    const int l = wv >> 2, s = wv & 3;
    return W + (size_t)(munit0(l) + 2 * s * mkb(l)) * 128 + (threadIdx.x & 63);
}
template <int L, int S, class Lay = RingLay, int HB = 0, int NH = 2, bool PRE = false>
__device__ __forceinline__ void layer_role(unsigned char* lds, int qa, int L1, int nch, bool edge,
                                           const u32x4* __restrict__ W, const float* __restrict__ bias,
                                           unsigned char* __restrict__ u2row, int xown,
                                           const u32x4 (*pre)[1][2] = nullptr) {
    constexpr int NKB = mkb(L);
    constexpr bool PL = L == 0 && Lay::PLANES;
    static_assert(NH * NKB >= kPre, "a role holds at least the handed-over k-blocks");
    constexpr int IN_OFF = L == 0 ? Lay::R0_OFF : (L == 1 ? Lay::R1_OFF : Lay::R2_OFF);
    constexpr int LO_IN = L == 0 ? 128 : 256;           // lo half offset in an input row
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
    u32x4 a[NH][NKB][2];
    float bv[NH][4];
#pragma unroll
    for (int hh = 0; hh < NH; ++hh) {
        const int h = HB + hh;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            const int u = munit0(L) + (2 * S + h) * NKB + kb;
            if (PRE && hh * NKB + kb < kPre) {
                a[hh][kb][0] = pre[hh * NKB + kb][0][0];
                a[hh][kb][1] = pre[hh * NKB + kb][0][1];
            } else {
                a[hh][kb][0] = W[u * 128 + lane];
                a[hh][kb][1] = W[u * 128 + 64 + lane];
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[hh][r] = bias[L * 128 + 32 * S + 16 * h + 4 * g + r];
    }
    unsigned radr[NKB][4], xadr[4], oadr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            const MSlot sl = mslot(L, S, kb, g);  // the input ring runs one column ahead of this layer
            if constexpr (PL) {
                const int e0 = li + sl.dq + 3, v = e0 & 3, row0 = (e0 >> 2) + (v >= 2 ? 1 : 0);  // chunk 0
                radr[kb][j] = Lay::U_OFF + (v * PROWS + row0) * PRS + 16 * (sl.oct ^ (((row0 >> 2) + j) & 1));
            } else {
                const int row = (16 * j + li + sl.dq - 1) & (RROWS - 1);
                radr[kb][j] = IN_OFF + (L == 0 ? row * RS0 + sl.oct * 16 : r12_at(row, sl.oct));
            }
        }
        xadr[j] = Lay::R1_OFF + r12_at((16 * j + li - 2) & (RROWS - 1), 4 * S + g);
        // unit 4S + 16 (g & 1) + (g >> 1) (+ 2h below: bit 1, so the swap of bit 0 commutes)
        oadr[j] = (L == 0 ? Lay::R1_OFF : Lay::R2_OFF) +
                  r12_at((16 * j + li) & (RROWS - 1), 4 * S + 16 * (g & 1) + (g >> 1));
    }
    u32x4 aid[NH];  // identity A of m-block h: row li takes fragment row 16h + li = 8g + e
#pragma unroll
    for (int hh = 0; hh < NH; ++hh) {
        h8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (_Float16)(16 * (HB + hh) + li == 8 * g + e ? 1.f : 0.f);
        aid[hh] = __builtin_bit_cast(u32x4, v);
    }
    const int sL = qa + 2 - L;
    auto work = [&](int k, auto jc) {
        constexpr int j = decltype(jc)::value;
        const unsigned adv = PL ? (unsigned)(k * 4 * PRS) : 0u;  // 16 columns = 4 rows of every plane
        u32x4 bh[NKB], bl[NKB];
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            bh[kb] = *reinterpret_cast<const u32x4*>(lds + (radr[kb][j] + adv));
            bl[kb] = *reinterpret_cast<const u32x4*>(lds + (radr[kb][j] + adv) + LO_IN);
        }
        u32x4 xh, xl;
        if constexpr (L == 2) {
            xh = *reinterpret_cast<const u32x4*>(lds + xadr[j]);
            xl = *reinterpret_cast<const u32x4*>(lds + xadr[j] + 256);
        }
        f32x4 acc[NH];
#pragma unroll
        for (int h = 0; h < NH; ++h) acc[h] = f32x4{bv[h][0], bv[h][1], bv[h][2], bv[h][3]};
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int pr = 0; pr < 3; ++pr)
#pragma unroll
                for (int h = 0; h < NH; ++h) acc[h] = mfma_h(a[h][kb][pr == 2], pr == 1 ? bl[kb] : bh[kb], acc[h]);
        if constexpr (L == 2) {
#pragma unroll
            for (int h = 0; h < NH; ++h) acc[h] = mfma_h(aid[h], xh, acc[h]);
#pragma unroll
            for (int h = 0; h < NH; ++h) acc[h] = mfma_h(aid[h], xl, acc[h]);
        }
        const int x0 = sL + 16 * k;  // this chunk's first column
        const bool straddle = edge && (x0 < 0 || x0 + 16 > L1);  // wave-uniform
#pragma unroll
        for (int hh = 0; hh < NH; ++hh) {
            const int h = HB + hh;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = acc[hh][r];
            if constexpr (L < 2) {
                leaky4(v);
                if (straddle) {
                    const int x = x0 + li;
                    if (x < 0 || x >= L1) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = 0.f;
                    }
                }
            }
            unsigned h0, h1, l0, l1;
            split2u(v[0], v[1], h0, l0);
            split2u(v[2], v[3], h1, l1);
            // lane groups 0/1 (2/3): channels 0-7 (8-15) of the m-block as
            // one 16-B hi chunk (group 0/2) and one lo chunk (group 1/3)
            const auto s0 = __builtin_amdgcn_permlane16_swap(h0, l0, false, false);
            const auto s1 = __builtin_amdgcn_permlane16_swap(h1, l1, false, false);
            const u32x4 val{s0[0], s1[0], s0[1], s1[1]};
            if constexpr (L < 2) {
                *reinterpret_cast<u32x4*>(lds + oadr[j] + 32 * h) = val;
            } else {
                const int x = x0 + li;
                if (k >= 0 && x >= 0 && x < xown)  // U2 row of position 4x + S
                    gstore16<M2_U2_STORE>(u2row, ((size_t)4 * x + S) * 128 + 32 * h + 64 * (g & 1) + 16 * (g >> 1),
                                          val);
            }
        }
    };
    const int LAST = nch + 2;  // conv2 computes chunk nch - 1 in step nch + 2
    auto step = [&](int s, auto jc) {
        if (s <= LAST) {
            const int k = s - (L + 1);
            if (k >= -1 && k < nch) work(k, jc);
            step_barrier();
        }
    };
    constexpr int J0 = (-1 - (L + 1)) & 3;  // ring phase of step -1's chunk
#pragma unroll 1
    for (int s = -1; s <= LAST; s += 4) {
        step(s, ic<J0>{});
        step(s + 1, ic<(J0 + 1) & 3>{});
        step(s + 2, ic<(J0 + 2) & 3>{});
        step(s + 3, ic<(J0 + 3) & 3>{});
    }
}

}  // namespace mp
}  // namespace m2
