// The vocoder's launch plan: which kernels one m2_vocoder call launches, with
// what grid, threads and LDS bytes.  Host arithmetic only - no HIP call and no
// sw(): the switch table and the device's workgroup slots are arguments, so
// tools/plan_check.cpp runs every rule on the CPU.  vocoder_run
// (m2_runtime.hip) plans once per call and the launchers (vocoder_x3.hip,
// vocoder_midp.hip, vocoder_tailp.hip, vocoder_tailp2.hip, vocoder_fused.hip)
// launch what the plan names.  (m2_model.h's VocoderPlan is the creation plan:
// the packs of a handle.)
//
// The tilings and LDS window plans of the split-f16 kernels (namespace x3) and
// of the exact-f32 kernels live here, because the plan needs their windows,
// waves and LDS bytes and the kernels take the same types as template
// arguments.
//
// The printed form of a plan (VocLaunchPlan::print, m2_debug_vocoder_plan) is
// one line of space-separated items, fixed:
//   perlayer
//   split  stage=1|2 headmid[n= S= nch= trans= G] | head[tf= comp= trans= G]  then
//          midp[nch= G] | x3mid[alt= w= G]   (absent after headmid[...])  then
//          tailp[nl= nch= G] | tailp2[nl= nch= G] | x3tail[alt= w= G]  then
//          redo=none|in-tail|host|guarded[FORM pair= comp= thr= lds=]  then,
//          when the call is kept off the fused head + mid launch,
//          no-headmid="<reason>"
//   f32    stage=0|1|2 form=FORM pair= comp= trans= head[tf= G] mid[w= G] tail[w= G] redo=none
// with G = grid=<x>x<y> thr=<threads> lds=<bytes> and FORM one of kF32Forms'
// names.  Every field of the plan is on the line.
#pragma once
#include <cstdint>
#include <cstdio>

#include "m2_common.h"

namespace m2 {

// ---------------------------------------------------------------------------
// Strip length of the pipelined kernels (16-column chunks per workgroup): the
// one in [nmin, 256] minimising rounds of wgs_per_round workgroups x (strip +
// extra_steps pipeline steps), the shortest on a tie.
namespace pipe {
struct StripRule {
    int nmin, wgs_per_round, extra_steps;
};
inline int pick_strip(int chunks, int B, int nmin, int wgs_per_round, int extra_steps) {
    int nch = 0;
    long best = -1;
    for (int n = nmin; n <= 256; ++n) {
        const long wgs = (long)cdiv(chunks, n) * B, rounds = (wgs + wgs_per_round - 1) / wgs_per_round;
        const long cost = rounds * (n + extra_steps);
        if (best < 0 || cost < best) best = cost, nch = n;
    }
    return nch;
}
inline int pick_strip(int chunks, int B, StripRule r) {
    return pick_strip(chunks, B, r.nmin, r.wgs_per_round, r.extra_steps);
}
// The three pipelines' rules, nl the number of computing layers (6 or 7).
// midp: rounds of 256 workgroups (one per CU; stage1 B = 32, L1 = 2000: 8
// strips of 16 chunks, one round; the round-4 sweep at 8 / 16 / 32 measured
// 23.1 / 20.0 / 29.9 us).
constexpr StripRule kMidpStrip{4, 256, 4};
// tailp: rounds of 768 workgroups (three per CU; stage1 B = 32, L2 = 8000: 24
// strips of 21 chunks, one round; B = 8: 63 strips of 8).
constexpr StripRule tailp_strip(int nl) { return {8, 768, nl + 1}; }
// tailp2: one workgroup per CU, any length from 8 to 256 (the kernel takes it
// at run time: 16 x 2600 gets 256 strips of 163 chunks, one round, where the
// instantiated lengths of round 4 gave 224 strips of 192).
constexpr StripRule tailp2_strip(int nl) { return {8, 256, nl}; }
// A forced length (M2_MIDP_NCH, M2_TAILP_NCH, M2_TAILP2_NCH) is clamped here.
constexpr int kMaxForcedStrip = 4096;
// Threads and LDS bytes of the pipelined kernels (each .hip asserts its own).
constexpr int kMidpThreads = 13 * 64, kMidpLds = 88064;
constexpr int tailp_threads(int nl) { return (nl + 1) * 64; }
constexpr int tailp_lds(int nl) { return nl == 6 ? 49184 : 55312; }
constexpr int tailp2_threads(int nl) { return (nl == 6 ? 12 : 14) * 64; }
constexpr int tailp2_lds(int nl) { return nl == 6 ? 98352 : 110608; }
}  // namespace pipe

// ---------------------------------------------------------------------------
// Split-f16 kernels (vocoder_x3.hip).
namespace x3 {

// Row stride in bytes for C channels: >= 4C, multiple of 16, (RS/16) % 4 == 2
// (C = 8: 32 B, 2-way conflicts between rows 8 apart are accepted).
constexpr int rs_for(int C) {
    int u = (4 * C + 15) / 16;
    if (C <= 8) return u * 16;
    while (u % 4 != 2) ++u;
    return u * 16;
}
constexpr int rup16(int n) { return (n + 15) / 16 * 16; }
constexpr int cmax(int a, int b) { return a > b ? a : b; }

// Two LDS regions per kernel, A then B, with buffers aliased by lifetime.
// Region-A buffers are sized to the rows actually written; the garbage
// columns of a partial 16-wide tile may read past them into region B, which
// only feeds columns that are never stored (an MFMA output column depends
// on its own B column only).  Region-B buffers keep the full read extent.
template <int MP, int C, int TF, bool PL = false>
struct HeadPlan {  // A: a0 | h   B: mel | u
    static constexpr int C1 = C / 2;
    static constexpr int RS_M = rs_for(MP), RS_C = rs_for(C), RS_1 = rs_for(C1);
    static constexpr int MEL_N = TF + 6, A0_N = TF + 4, NQ = TF + 2, H_N = 4 * TF + 2, O_N = 4 * TF;
    static constexpr int CAP_MEL = cmax(MEL_N, rup16(A0_N) + 2);
    static constexpr int CAP_U = cmax(4 * NQ, rup16(H_N) + 4);
    // PL: the phase-planar path keeps h and u as 4 planes of 64 rows
    static constexpr int RA = cmax(A0_N * RS_C, cmax(H_N, PL ? 4 * 64 : 0) * RS_1);
    static constexpr int LDS_BYTES = RA + cmax(CAP_MEL * RS_M, cmax(CAP_U, PL ? 4 * 64 + 4 : 0) * RS_1);
};

template <int CI, int W>
struct MidPlan {  // A: in | h   B: u
    static constexpr int CO = CI / 2;
    static constexpr int RS_I = rs_for(CI), RS_O = rs_for(CO);
    static constexpr int IN_N = W + 4, NQ = W + 2, H_N = 4 * W + 2, O_N = 4 * W;
    static constexpr int CAP_U = cmax(4 * NQ, rup16(H_N) + 4);
    static constexpr int RA = cmax(IN_N * RS_I, H_N * RS_O);
    static constexpr int LDS_BYTES = RA + CAP_U * RS_O;
};

template <int CI, int W>
struct TailPlan {  // A: in | h3 | u4   B: u3 | h4
    static constexpr int C3 = CI / 2, C4 = CI / 4;
    static constexpr int RS_I = rs_for(CI), RS_3 = rs_for(C3), RS_4 = rs_for(C4);
    static constexpr int IN_N = W + 8, NQ3 = W + 6, H3_N = 2 * W + 8, O3_N = 2 * W + 6;
    static constexpr int NQ4 = 2 * W + 4, H4_N = 4 * W + 4, O4_N = 4 * W + 2, A_N = 4 * W;
    static constexpr int CAP_U3 = cmax(2 * NQ3, cmax(rup16(H3_N) + 3, rup16(NQ4) + 5));
    static constexpr int CAP_H4 = cmax(H4_N, rup16(O4_N) + 2);
    static constexpr int RA = cmax(IN_N * RS_I, cmax(H3_N * RS_3, 2 * NQ4 * RS_4));
    static constexpr int LDS_BYTES = RA + cmax(CAP_U3 * RS_3, CAP_H4 * RS_4);
};

// Tilings.  Per kernel: waves per workgroup (*W), window (TF frames / W2 /
// W3 positions), launch-bound waves per SIMD (*MIN: 4 -> <= 128 VGPRs), and
// NT_* = tile-chunk size per layer, chosen so each layer's items come to a
// multiple of the wave count.  Stage1 at B=32, T=500 (bench): head 8 x 32 =
// 256 workgroups (one per CU), mid 16 x 32 = 512 (two rounds), tail 48 x 32 =
// 1536 at two per CU (three full rounds).
struct CfgS1 {
    static constexpr int PDM = 4;
    static constexpr int M = 64, MP = 64, C = 128;
    static constexpr int TF = 63, HW = 16, HMIN = 4;
    static constexpr int W2 = 125, MW = 16, MMIN = 4;
    static constexpr int W3 = 168, TW = 8, TMIN = 4;
    static constexpr int NT_IN = 3, NT_T1 = 5, NT_R1 = 4, NT_T2 = 4, NT_R2 = 4, NT_T3 = 3, NT_R3 = 3, NT_T4 = 3,
                         NT_R4 = 6;
};
#ifndef X3S2_TF  // stage2 tiling experiments (tools/probe/s2_tiles.sh)
#define X3S2_TF 16
#define X3S2_NT_R1 5
#endif
#ifndef X3S2_W2
#define X3S2_W2 30
#define X3S2_NT_R2 4
#endif
#ifndef X3S2_W3
#define X3S2_W3 120
#define X3S2_NT_T3 4
#define X3S2_NT_R3 4
#endif
struct CfgS2 {
    static constexpr int M = 80, MP = 96, C = 256;
    static constexpr int TF = X3S2_TF, HW = 8, HMIN = 2;
    static constexpr int W2 = X3S2_W2, MW = 8, MMIN = 2;
    static constexpr int W3 = X3S2_W3, TW = 8, TMIN = 2;
    static constexpr int NT_IN = 2, NT_T1 = 2, NT_R1 = X3S2_NT_R1, NT_T2 = 4, NT_R2 = X3S2_NT_R2, NT_T3 = X3S2_NT_T3,
                         NT_R3 = X3S2_NT_R3, NT_T4 = 4, NT_R4 = 4;
    // weight k-blocks in flight per item (8 VGPRs each).  4, as stage1: 8 and
    // 12 (the 256-VGPR budget of 8 waves at one workgroup per CU allows them)
    // measured level or slower - head 25.8 / 26.3 / 27.0 us at 8x500, mid
    // 184.2 / 184.4 / 185.2 us at 16x2600 (profiles/r04/r04b_pdm_pipeline_ab.txt):
    // the stage2 head and mid are not bound by the latency of their weight
    // stream
    static constexpr int PDM = 4;
    // head B fragments one k-block ahead (mma_x3 BP; 116 -> 156 VGPRs, one
    // workgroup per CU either way): head 26.5 -> 25.0 us at 8x500; in the mid
    // kernels it measured slower (24.0 -> 26.0 us at 8x500, 186 -> 212 us at
    // 16x2600: 4 -> 3 waves per SIMD), in the 16-wave H24 head level (172 ->
    // 175 us, spills; its hi-only form, BP 2, 173.6 -> 171.5 us: CfgS2H24) -
    // profiles/r05/r05g_bpipe_ab.txt, r05r_head_bp2_ab.txt
    static constexpr int HBP = 1;
};
// Stage2 mid / tail tilings for small grids (plan_vocoder_launch picks per
// call): at B=8, T=500 the default windows make 576 mid workgroups (1.1 rounds
// of 512 slots at two per CU) and 536 tail workgroups (2.1 rounds of 256 at
// one per CU); 32 / 125 make 504 and 512 (one and two full rounds), at 1.20x /
// 1.075x the time per workgroup (5-tile chunks where 4 were enough).
// Measured B=8 T=500: mid 26.4 -> 22.9 us, tail 35.5 -> 26.1 us; large grids
// keep the defaults (tools/probe/s2_tiles.sh).  Since round 5 the windows
// are 30 and 33 positions (same tiles, fewer workgroups: below).
struct CfgS2Alt : CfgS2 {
    static constexpr int W2 = 33, NT_R2 = 5;
    static constexpr int W3 = 125, NT_T3 = 5, NT_R3 = 5;
};
constexpr double kAltMidCost = 1.20, kAltTailCost = 1.075;
// Stage2 head windows of 24 frames for large grids (composed head: less
// weight streaming per frame; 16x2600 0.569 -> 0.548 ms, 64x500 0.430 ->
// 0.421 ms per vocoder step, but 8x500 0.072 -> 0.075 ms: 168 workgroups
// leave CUs idle), taken when the 16-frame grid has >= 1024 workgroups.
// 16 waves per workgroup there (more latency hiding at one workgroup per CU:
// head 140.8 -> 135.2 us at 64x500, 170.6 -> 165.4 at 16x2600; at 8x500 the
// 16-frame, 8-wave head stays).
struct CfgS2H24 : CfgS2 {
    static constexpr int TF = 24, HW = 16;
    static constexpr int PDM = 4;  // 16 waves: 128 VGPRs per wave
    static constexpr int HBP = 2;  // B fragments ahead, hi halves only (CfgS2::HBP)
};
constexpr long kS2WideHeadWGs = 1024;  // in 16-frame windows
// Each window's layers run whole 16-row m-tiles: the head's ResBlock1 covers
// 4 TF + 2 rows (16 and 19 frames: 5 tiles, 24 and 27: 7), the mid's
// ResBlock2 4 W + 2 and its ConvT2 W + 2 rows per phase (28 and 30
// positions: 8 and 2 tiles, 32 and 33: 10 with NT_R2 = 5, and 3).  So the
// 19 / 27-frame heads and the 30 / 33-position mids cost what the 16 / 24 /
// 28 / 32 ones do per workgroup and make fewer workgroups; the plan takes
// the fewer rounds of workgroup slots, the smaller window when the rounds tie.
// Bit-identical audio either way (every output sums the same products in the
// same order).  Alternated twice (profiles/r05/r05ab_windows_ab.txt): head
// 38.9 -> 27.2 us at 16x262 (272 -> 224 workgroups: one round of 256),
// 146.3 -> 132.9 at 128x262, 141.2 -> 128.0 at 64x500; mid 184.4 -> 176.6 us
// at 16x2600, 149.1 -> 145.2 at 128x262, 26.7 -> 25.2 at 16x262 (W33:
// 512 workgroups, one round of two per CU).
struct CfgS2T19 : CfgS2 {
    static constexpr int TF = 19;
};
struct CfgS2H27 : CfgS2H24 {
    static constexpr int TF = 27;
};

// The stage1 head runs ConvT1 / ResBlock1 phase-planar when one item per wave
// covers them: planes of 64 rows hold TF + 2 <= 65 input columns and the
// (phase, m-block) items of the C/2-channel layers number exactly HW.
template <class Cfg>
constexpr bool head_planar() {
    return Cfg::TF + 1 <= 64 && 4 * (Cfg::C / 2 / 16) == Cfg::HW;
}
template <class Cfg>
using HeadPlanOf = HeadPlan<Cfg::MP, Cfg::C, Cfg::TF, head_planar<Cfg>()>;

// headmid_kernel (stage1 head + mid in one launch): a workgroup owns a strip
// of S <= S_MAX columns of U1; owned columns + one on either side = the 4 TF
// valid positions of the head's planes.
constexpr int kHeadmidSMax = 4 * CfgS1::TF - 2;
constexpr int kHeadmidLds = HeadPlan<CfgS1::MP, CfgS1::C, CfgS1::TF, true>::LDS_BYTES;

}  // namespace x3

// ---------------------------------------------------------------------------
// Exact-f32 kernels (vocoder_fused.hip): tilings.  WAVES waves per workgroup;
// NT_* = 16-position tiles per work item of each layer, chosen so every layer
// splits into a multiple of WAVES items; MINW = launch-bounds waves per SIMD
// (VGPR cap).
struct CfgS1W8 {  // stage1: 8 waves, <= 74 KB LDS (2 workgroups / CU)
    static constexpr int M = 64, C = 128, TF = 28, W2 = 60, W3 = 240, WAVES = 8, MINW = 5;
    static constexpr bool CP = false;
    static constexpr int NT_IN = 2, NT_T1 = 2, NT_R1 = 4, NT_T2 = 4, NT_R2 = 4, NT_T3 = 4, NT_R3 = 4, NT_T4 = 4, NT_R4 = 4;
};
struct CfgS1W16 {  // stage1: 16 waves, one workgroup per CU (152/132/131 KB LDS)
    static constexpr int M = 64, C = 128, TF = 63, W2 = 125, W3 = 500, WAVES = 16, MINW = 4;
    static constexpr bool CP = false;
    static constexpr int NT_IN = 3, NT_T1 = 5, NT_R1 = 4, NT_T2 = 4, NT_R2 = 4, NT_T3 = 4, NT_R3 = 4, NT_T4 = 8, NT_R4 = 8;
};
struct CfgS1W16s {  // CfgS1W16 with ~2-3 smaller work items per wave for the dynamic schedule
    static constexpr int M = 64, C = 128, TF = 63, W2 = 125, W3 = 500, WAVES = 16, MINW = 4;
    static constexpr bool CP = false;
    static constexpr int NT_IN = 2, NT_T1 = 2, NT_R1 = 2, NT_T2 = 2, NT_R2 = 2, NT_T3 = 2, NT_R3 = 2, NT_T4 = 4, NT_R4 = 4;
};
// The 16-wave tiling's mid and tail as two 8-wave workgroups per CU (the
// windows halved: 1,024 workgroups at B=32 T=500, two rounds as before), so
// one workgroup's layer barriers overlap the other's MFMA chains (M2_F32_MT).
// Measured in one process, B=32 T=500 with the two-phase tail layers
// (profiles/r06/r06z3_mt.txt): the tail 0.1986 -> 0.1948 ms per call (the
// default, M2_F32_MT=2); the mid 0.228 (its 63-position windows re-read
// twice the halo).
struct CfgS1T8 {
    static constexpr int M = 64, C = 128, TF = 28, W2 = 63, W3 = 250, WAVES = 8, MINW = 5;
    static constexpr bool CP = false;
    static constexpr int NT_IN = 2, NT_T1 = 2, NT_R1 = 4, NT_T2 = 4, NT_R2 = 4, NT_T3 = 4, NT_R3 = 4, NT_T4 = 4, NT_R4 = 4;
};
struct CfgS2W8 {
    static constexpr int M = 80, C = 256, TF = 12, W2 = 28, W3 = 120, WAVES = 8, MINW = 5;
    static constexpr bool CP = false;
    static constexpr int NT_IN = 2, NT_T1 = 2, NT_R1 = 4, NT_T2 = 4, NT_R2 = 4, NT_T3 = 4, NT_R3 = 4, NT_T4 = 4, NT_R4 = 4;
};
struct CfgTinyW8 {  // M2TTSModel(hidden 32, mel 32, vocoder 64) as in the reference smoke tests
    static constexpr int M = 32, C = 64, TF = 28, W2 = 60, W3 = 240, WAVES = 8, MINW = 5;
    static constexpr bool CP = false;
    static constexpr int NT_IN = 2, NT_T1 = 2, NT_R1 = 4, NT_T2 = 4, NT_R2 = 4, NT_T3 = 4, NT_R3 = 4, NT_T4 = 4, NT_R4 = 4;
};

namespace f32 {
constexpr int rup16(int n) { return (n + 15) / 16 * 16; }
// Row stride >= cols with stride = 16 (mod 32): conflict-free B-operand reads.
constexpr int pstride(int cols) { return ((cols + 15) / 32) * 32 + 16; }
constexpr int cmax(int a, int b) { return a > b ? a : b; }
// Compact row stride (multiple of 4, >= cols): up to 4-lane 2-way conflicts
// between the two 16-lane halves of a read, in exchange for LDS capacity.
constexpr int cstride(int cols) { return (cols + 3) / 4 * 4 + ((((cols + 3) / 4 * 4) % 32 == 0) ? 4 : 0); }
constexpr int stride_for(int cols, bool compact) { return compact ? cstride(cols) : pstride(cols); }
// Odd row stride >= cols (the two-phase layers' stride-2 B reads).
constexpr int ostride(int cols) { return ((cols + 15) / 32) * 32 + 17; }

// Window plans.  All column counts are exact receptive-field arithmetic; the
// capacities also cover the garbage columns a 16-wide MFMA tile computes past
// the last needed position (those columns are never stored).
template <int M, int C, int TF, bool CP = false>
struct HeadPlan {
    static constexpr int C1 = C / 2;
    static constexpr int MEL_N = TF + 6;           // frames [f0-3, f0+TF+3)
    static constexpr int A0_N = TF + 4;            // input conv out  [f0-2, f0+TF+2)
    static constexpr int NQ = TF + 2;              // ConvT1 inputs   [f0-1, f0+TF+1)
    static constexpr int H_N = 4 * TF + 2;         // RB1 conv1 out   [4f0-1, 4f0+4TF+1)
    static constexpr int O_N = 4 * TF;             // RB1 out         [4f0, 4f0+4TF)
    static constexpr int P_MEL = stride_for(cmax(MEL_N, rup16(A0_N) + 2), CP);
    static constexpr int P_A0 = stride_for(cmax(A0_N, rup16(NQ) + 2), CP);
    static constexpr int P_U = stride_for(cmax(4 * NQ, rup16(H_N) + 4), CP);
    static constexpr int P_H = stride_for(cmax(H_N, rup16(O_N) + 2), CP);
    static constexpr int R0 = cmax(M * P_MEL + C * P_A0, C1 * P_H);
    static constexpr int R1 = C1 * P_U;
    static constexpr int LDS_FLOATS = R0 + R1;
};

template <int CI, int W>
struct MidPlan {  // U1 (CI ch, res 4) -> U2 (CI/2 ch, res 16); W res-4 positions
    static constexpr int CO = CI / 2;
    static constexpr int IN_N = W + 4;             // [p0-2, p0+W+2)
    static constexpr int NQ = W + 2;               // ConvT2 inputs [p0-1, p0+W+1)
    static constexpr int H_N = 4 * W + 2;          // [4p0-1, 4p0+4W+1)
    static constexpr int O_N = 4 * W;              // [4p0, 4p0+4W)
    static constexpr int P_IN = pstride(cmax(IN_N, rup16(NQ) + 2));
    static constexpr int P_U = pstride(cmax(4 * NQ, rup16(H_N) + 4));
    static constexpr int P_H = pstride(cmax(H_N, rup16(O_N) + 2));
    static constexpr int R0 = cmax(CI * P_IN, CO * P_H);
    static constexpr int R1 = CO * P_U;
    static constexpr int LDS_FLOATS = R0 + R1;
};

template <int CI, int W, bool PAIR = false>
struct TailPlan {  // U2 (CI ch, res 16) -> audio (res 64); W res-16 positions
    static constexpr int C3 = CI / 2, C4 = CI / 4;
    static constexpr int IN_N = W + 8;             // [p0-4, p0+W+4)
    static constexpr int NQ3 = W + 6;              // ConvT3 inputs [p0-3, p0+W+3) -> U3 [2p0-6, ..)
    static constexpr int H3_N = 2 * W + 8;         // [2p0-4, 2p0+2W+4)
    static constexpr int O3_N = 2 * W + 6;         // [2p0-3, 2p0+2W+3)
    static constexpr int NQ4 = 2 * W + 4;          // ConvT4 inputs [2p0-2, 2p0+2W+2) -> U4 [4p0-4, ..)
    static constexpr int H4_N = 4 * W + 4;         // [4p0-2, 4p0+4W+2)
    static constexpr int O4_N = 4 * W + 2;         // [4p0-1, 4p0+4W+1)
    static constexpr int A_N = 4 * W;              // audio [4p0, 4p0+4W)
    static constexpr int P_IN = pstride(cmax(IN_N, rup16(NQ3) + 2));
    static constexpr int P_U3 = pstride(cmax(2 * NQ3, cmax(rup16(H3_N) + 3, rup16(NQ4) + 5)));
    static constexpr int P_H3 = pstride(cmax(H3_N, rup16(O3_N) + 2));
    // (PAIR: the two-phase ResBlock4 reads up to 2 x 16 columns past its last
    // needed position pair)
    static constexpr int P_U4 = PAIR ? ostride(cmax(2 * NQ4, 4 * W + 40)) : pstride(cmax(2 * NQ4, rup16(H4_N) + 3));
    static constexpr int P_H4 = PAIR ? ostride(cmax(H4_N, 4 * W + 40)) : pstride(cmax(H4_N, rup16(O4_N) + 2));
    // region A: U2in -> H3 -> U4 ; region B: U3 -> H4
    static constexpr int RA = cmax(CI * P_IN, cmax(C3 * P_H3, C4 * P_U4));
    static constexpr int RB = cmax(C3 * P_U3, C4 * P_H4);
    static constexpr int LDS_FLOATS = RA + RB;
};

// A tiling as the plan sees it: windows, threads, LDS bytes per kernel (the
// tail's with and without the two-phase layers).
struct Tiling {
    const char* name;
    int tf, w2, w3, threads, head_lds, mid_lds, tail_lds[2];
};
template <class Cfg>
constexpr Tiling tiling_of(const char* name) {
    return {name,
            Cfg::TF,
            Cfg::W2,
            Cfg::W3,
            Cfg::WAVES * 64,
            4 * HeadPlan<Cfg::M, Cfg::C, Cfg::TF, Cfg::CP>::LDS_FLOATS,
            4 * MidPlan<Cfg::C / 2, Cfg::W2>::LDS_FLOATS,
            {4 * TailPlan<Cfg::C / 4, Cfg::W3, false>::LDS_FLOATS, 4 * TailPlan<Cfg::C / 4, Cfg::W3, true>::LDS_FLOATS}};
}
enum TilingId : int { S1W8, S1W16, S1W16s, S1T8, S2W8, TinyW8, kTilings };
constexpr Tiling kTiling[kTilings] = {tiling_of<CfgS1W8>("S1W8"),     tiling_of<CfgS1W16>("S1W16"),
                                      tiling_of<CfgS1W16s>("S1W16s"), tiling_of<CfgS1T8>("S1T8"),
                                      tiling_of<CfgS2W8>("S2W8"),     tiling_of<CfgTinyW8>("TinyW8")};

// The (head, mid, tail) tilings a call can take, as one enumerator; redo: the
// guarded redo's tiling, the 8-wave form of the stage (every stage1 tiling
// packs the same weights and writes the same U1 / U2 / audio), so it gets up
// to 256 VGPRs per lane at one workgroup per CU.
enum Form : int { S1_W16S, S1_W16_MT0, S1_W16_MT1, S1_W16_MT2, S1_W16_MT3, S1_W16_MT4, S1_W8, S2_W8, TINY_W8, kForms };
struct FormRow {
    const char* name;
    TilingId head, mid, tail, redo;
};
constexpr FormRow kF32Forms[kForms] = {
    {"S1_W16S", S1W16s, S1W16s, S1W16s, S1W8},
    {"S1_W16_MT0", S1W16, S1W16, S1W16, S1W8},
    {"S1_W16_MT1", S1W16, S1T8, S1W16, S1W8},
    {"S1_W16_MT2", S1W16, S1W16, S1T8, S1W8},
    {"S1_W16_MT3", S1W16, S1T8, S1T8, S1W8},
    // the mid's items halved (two per wave), the tail on half windows: 0.1843 -> 0.1894 ms
    // alternated (profiles/r06/r06z14_mid_items.txt), a switch only
    {"S1_W16_MT4", S1W16, S1W16s, S1T8, S1W8},
    {"S1_W8", S1W8, S1W8, S1W8, S1W8},
    {"S2_W8", S2W8, S2W8, S2W8, S2W8},
    {"TINY_W8", TinyW8, TinyW8, TinyW8, TinyW8},
};
// Workgroup slots the 16-wave / 8-wave stage1 heads are judged by: one 16-wave
// workgroup per CU, 8-wave workgroups pair up.
constexpr int kSlotsW16 = 256, kSlotsW8 = 512;
}  // namespace f32

// ---------------------------------------------------------------------------
// What a call is.
struct VocCall {
    int M = 0, C = 0;  // (mel_channels, vocoder_channels)
    int B = 0, T = 0;  // T: the frame count, or the capacity when it is on the device
    bool trans = false;     // mel is [B, T, M]
    bool device_T = false;  // the frame count is a device word (speculative launch)
    unsigned prof_slots = 0;  // kernels (bits 0..2) this call records events around
    // the packs of the handle
    bool hc = false, mp = false, tp = false, tp2 = false, redo_w = false;  // split-f16 (VocX)
    bool wt4p = false, hcw = false;                                        // exact-f32 (VocW)
    bool fused = false;  // the handle has the fused kernels (else: per layer)
    bool x3 = false;     // the call runs on the split-f16 kernels
    int range_policy = 0;  // 0 report, 1 fallback
    int redo = -1;         // policy 1: the call's device flag word (0 / 1), -1: none
};

// Workgroup slots of the device (CUs x occupancy) per split-f16 tiling that a
// rule weighs.  The GPU build queries them once (vocoder_x3.hip:
// vocoder_x3_slots); tools/plan_check.cpp passes numbers.
struct VocSlots {
    long head16, head19, head24, head27, mid, mid_alt, tail, tail_alt;
};

enum class VocPath { PerLayer, F32, Split };
enum class VocRedoPlan { None, InTail, Guarded, Host };
enum class VocHead : int { S1, S2T16, S2T19, S2H24, S2H27 };
enum class VocMid { Midp, X3, X3Alt };
enum class VocTail { Tailp, Tailp2, X3, X3Alt };

struct VocGrid {
    int x = 0, y = 0, threads = 0, lds = 0;
};

struct VocLaunchPlan {
    VocPath path = VocPath::PerLayer;
    int stage = 0;  // 1 / 2: the stage1 / stage2 shapes, 0: others (exact-f32 only)
    bool trans = false;
    // split
    bool headmid = false;
    const char* no_headmid = nullptr;  // why not (null when headmid, or off the split path)
    int hm_n = 0, hm_S = 0, hm_nch = 0;
    VocHead head = VocHead::S1;
    int head_tf = 0;
    bool comp = false;
    VocMid mid = VocMid::X3;
    int mid_nch = 0, mid_w = 0;
    VocTail tail = VocTail::X3;
    int tail_nl = 0, tail_nch = 0, tail_w = 0;
    // exact-f32 (the path itself, or the guarded redo behind the split kernels)
    f32::Form form = f32::S1_W8;
    bool pair = false, f32_comp = false;
    VocRedoPlan redo = VocRedoPlan::None;
    // launches: head (or headmid), mid (threads 0 after headmid), tail; redo_g: the guarded
    // launch's threads and LDS (its grid is the device's, voc_redo in vocoder_fused.hip)
    VocGrid head_g, mid_g, tail_g, redo_g;

    int print(char* out, size_t cap) const;
};

// Which mid / tail kernel family a handle's split path takes (the window of
// the x3 kernels is per call: plan_vocoder_launch).
inline VocMid voc_mid_kind(bool mp) { return mp ? VocMid::Midp : VocMid::X3; }
inline VocTail voc_tail_kind(bool tp, bool tp2) { return tp2 ? VocTail::Tailp2 : (tp ? VocTail::Tailp : VocTail::X3); }

// Why a call does not take headmid_kernel (null: it does).
inline const char* headmid_excluded(const VocCall& c, const Switches& s, bool comp) {
    if (!s.headmid) return "M2_HEADMID=0";
    if (!(c.M == 64 && c.C == 128)) return "not the stage1 shapes";
    if (c.device_T) return "the frame count is on the device: the grid covers the capacity";
    if (!c.mp || !c.hc || !comp) return "no split packs of the composed head and the pipelined mid (or M2_HEAD_INCONV)";
    if (s.midp_nch > 0) return "M2_MIDP_NCH forces the mid's strip length";
    if (c.prof_slots & 3u) return "events around the head or the mid: the fused launch has no boundary between them";
    return nullptr;
}

namespace detail {
inline long rounds_of(long n, long slots) { return (n + slots - 1) / slots; }
inline int strip_of(int forced, int chunks, int B, pipe::StripRule r) {
    return forced > 0 ? (forced < pipe::kMaxForcedStrip ? forced : pipe::kMaxForcedStrip) : pipe::pick_strip(chunks, B, r);
}
template <class Cfg>
constexpr VocGrid x3_head_grid() {
    return {0, 0, Cfg::HW * 64, x3::HeadPlanOf<Cfg>::LDS_BYTES};
}
}  // namespace detail

// The exact-f32 form of a call (also the guarded redo's: kF32Forms[form].redo).
inline void plan_f32_form(const VocCall& c, const Switches& s, VocLaunchPlan* p) {
    if (c.M == 64 && c.C == 128) {
        // Workgroup rounds: one 16-wave WG per CU; 8-wave WGs pair up.  Pick the
        // tiling whose workgroup count wastes the least of its last round.
        const int n16 = c.B * cdiv(c.T, CfgS1W16::TF), n8 = c.B * cdiv(c.T, CfgS1W8::TF);
        const double waste16 = (double)cdiv(n16, f32::kSlotsW16) * f32::kSlotsW16 / n16,
                     waste8 = (double)cdiv(n8, f32::kSlotsW8) * f32::kSlotsW8 / n8;
        const bool w16 = s.voc_plan == 2 || (s.voc_plan < 0 && waste16 <= waste8);
        p->pair = s.f32_pair && c.wt4p;
        p->f32_comp = s.f32_comp && c.hcw;
        if (s.voc_plan == 3) p->form = f32::S1_W16S;
        else if (!w16) p->form = f32::S1_W8;
        else p->form = s.f32_mt >= 1 && s.f32_mt <= 4 ? (f32::Form)(f32::S1_W16_MT0 + s.f32_mt) : f32::S1_W16_MT0;
    } else if (c.M == 80 && c.C == 256) {
        p->form = f32::S2_W8;
        p->f32_comp = s.f32_comp && c.hcw;
    } else {
        p->form = f32::TINY_W8;
    }
}

inline VocLaunchPlan plan_vocoder_launch(const VocCall& c, const Switches& s, const VocSlots& sl) {
    using detail::rounds_of;
    VocLaunchPlan p;
    p.trans = c.trans;
    if (!c.fused) return p;
    const int B = c.B, T = c.T;
    const bool s1 = c.M == 64 && c.C == 128, s2 = c.M == 80 && c.C == 256;
    p.stage = s1 ? 1 : (s2 ? 2 : 0);
    if (!c.x3) {
        p.path = VocPath::F32;
        plan_f32_form(c, s, &p);
        const f32::FormRow& f = f32::kF32Forms[p.form];
        const f32::Tiling &h = f32::kTiling[f.head], &m = f32::kTiling[f.mid], &t = f32::kTiling[f.tail];
        p.head_g = {cdiv(T, h.tf), B, h.threads, h.head_lds};
        p.mid_g = {cdiv(4 * T, m.w2), B, m.threads, m.mid_lds};
        p.tail_g = {cdiv(16 * T, t.w3), B, t.threads, t.tail_lds[p.pair]};
        return p;
    }
    p.path = VocPath::Split;
    // the redo strategy of range policy 1: the pipelined tail redoes its own
    // non-finite strips in fp32 inside the launch; else the guarded exact-f32
    // launch behind the tail; without a device flag word the host waits and
    // re-runs the call
    if (c.redo >= 0) p.redo = c.redo_w && !s.redo_launch ? VocRedoPlan::InTail : VocRedoPlan::Guarded;
    else if (c.range_policy == 1) p.redo = VocRedoPlan::Host;
    if (p.redo == VocRedoPlan::Guarded) {
        plan_f32_form(c, s, &p);
        const f32::Tiling& r = f32::kTiling[f32::kF32Forms[p.form].redo];
        const int tail = r.tail_lds[p.pair];
        p.redo_g = {0, 0, r.threads, r.head_lds > r.mid_lds ? (r.head_lds > tail ? r.head_lds : tail)
                                                              : (r.mid_lds > tail ? r.mid_lds : tail)};
    }
    // the composed input_conv o ConvT1 head when packed (stage1; 22.1 -> 19.7
    // us, profiles/ab/r02l_head_comp.txt); M2_HEAD_INCONV=1 runs the two
    // layers (A/B and test switch, m2_common.h switch table)
    p.comp = c.hc && !s.head_inconv;

    // tail
    p.tail = voc_tail_kind(c.tp, c.tp2);
    if (p.tail == VocTail::Tailp2) {
        // M2_TAILP2_NCH forces the strip; M2_TAILP2_SEVEN=1 the seven-layer form
        p.tail_nl = s.tailp2_seven ? 7 : 6;
        p.tail_nch = detail::strip_of(s.tailp2_nch, cdiv(16 * T, 16), B, pipe::tailp2_strip(p.tail_nl));
        p.tail_g = {cdiv(16 * T, 16 * p.tail_nch), B, pipe::tailp2_threads(p.tail_nl), pipe::tailp2_lds(p.tail_nl)};
    } else if (p.tail == VocTail::Tailp) {
        // M2_TAILP_NCH forces the strip; M2_TAILP_SEVEN=1: ResBlock4 conv2 and
        // the output conv as two layers (the round-2 form; A/B and test switch)
        p.tail_nl = s.tailp_seven ? 7 : 6;
        p.tail_nch = detail::strip_of(s.tailp_nch, cdiv(16 * T, 16), B, pipe::tailp_strip(p.tail_nl));
        p.tail_g = {cdiv(16 * T, 16 * p.tail_nch), B, pipe::tailp_threads(p.tail_nl), pipe::tailp_lds(p.tail_nl)};
    } else {
        const bool alt = s2 && rounds_of((long)cdiv(16 * T, x3::CfgS2Alt::W3) * B, sl.tail_alt) * x3::kAltTailCost <
                                   (double)rounds_of((long)cdiv(16 * T, x3::CfgS2::W3) * B, sl.tail);
        if (alt) p.tail = VocTail::X3Alt;
        p.tail_w = alt ? x3::CfgS2Alt::W3 : (s2 ? x3::CfgS2::W3 : x3::CfgS1::W3);
        const int lds = alt  ? x3::TailPlan<x3::CfgS2Alt::C / 4, x3::CfgS2Alt::W3>::LDS_BYTES
                        : s2 ? x3::TailPlan<x3::CfgS2::C / 4, x3::CfgS2::W3>::LDS_BYTES
                             : x3::TailPlan<x3::CfgS1::C / 4, x3::CfgS1::W3>::LDS_BYTES;
        p.tail_g = {cdiv(16 * T, p.tail_w), B, (s2 ? x3::CfgS2::TW : x3::CfgS1::TW) * 64, lds};
    }

    // stage1, host-known T, split packs: the head and the mid in one launch
    // (headmid_kernel), n strips of S <= kHeadmidSMax columns per utterance
    p.no_headmid = headmid_excluded(c, s, p.comp);
    p.mid = voc_mid_kind(c.mp);
    if (!p.no_headmid) {
        p.headmid = true;
        p.hm_n = cdiv(4 * T, x3::kHeadmidSMax);
        p.hm_S = cdiv(4 * T, p.hm_n);
        p.hm_nch = cdiv(p.hm_S, 16);
        p.head_tf = x3::CfgS1::TF;
        p.head_g = {p.hm_n, B, x3::CfgS1::HW * 64, x3::kHeadmidLds};
        return p;
    }

    // head.  stage2, composed head: the 16-wave heads (24 / 27 frames) on large
    // grids, the 8-wave heads (16 / 19) below; within a pair the fewer rounds
    // of workgroup slots, the smaller window on a tie (M2_S2_HEAD_TF forces;
    // a value other than 16, 19 or 24 takes the 27-frame head)
    p.head = s1 ? VocHead::S1 : VocHead::S2T16;
    if (s2 && p.comp) {
        auto rounds = [&](int tf, long slots) { return rounds_of((long)cdiv(T, tf) * B, slots); };
        int hv;
        if (s.s2_head_tf) hv = s.s2_head_tf;
        else if ((long)cdiv(T, 16) * B >= x3::kS2WideHeadWGs) hv = rounds(27, sl.head27) < rounds(24, sl.head24) ? 27 : 24;
        else hv = rounds(19, sl.head19) < rounds(16, sl.head16) ? 19 : 16;
        p.head = hv == 16 ? VocHead::S2T16 : hv == 19 ? VocHead::S2T19 : hv == 24 ? VocHead::S2H24 : VocHead::S2H27;
    }
    switch (p.head) {
        case VocHead::S1: p.head_tf = x3::CfgS1::TF, p.head_g = detail::x3_head_grid<x3::CfgS1>(); break;
        case VocHead::S2T16: p.head_tf = x3::CfgS2::TF, p.head_g = detail::x3_head_grid<x3::CfgS2>(); break;
        case VocHead::S2T19: p.head_tf = x3::CfgS2T19::TF, p.head_g = detail::x3_head_grid<x3::CfgS2T19>(); break;
        case VocHead::S2H24: p.head_tf = x3::CfgS2H24::TF, p.head_g = detail::x3_head_grid<x3::CfgS2H24>(); break;
        case VocHead::S2H27: p.head_tf = x3::CfgS2H27::TF, p.head_g = detail::x3_head_grid<x3::CfgS2H27>(); break;
    }
    p.head_g.x = cdiv(T, p.head_tf);
    p.head_g.y = B;

    // mid
    if (p.mid == VocMid::Midp) {
        // M2_MIDP_NCH forces the strip
        p.mid_nch = detail::strip_of(s.midp_nch, cdiv(4 * T, 16), B, pipe::kMidpStrip);
        p.mid_g = {cdiv(4 * T, 16 * p.mid_nch), B, pipe::kMidpThreads, pipe::kMidpLds};
    } else {
        bool alt = false;
        if (s2 && s.s2_mid_alt >= 0) alt = s.s2_mid_alt == 1;
        else if (s2)
            alt = rounds_of((long)cdiv(4 * T, x3::CfgS2Alt::W2) * B, sl.mid_alt) * x3::kAltMidCost <
                  (double)rounds_of((long)cdiv(4 * T, x3::CfgS2::W2) * B, sl.mid);
        if (alt) p.mid = VocMid::X3Alt;
        p.mid_w = alt ? x3::CfgS2Alt::W2 : (s2 ? x3::CfgS2::W2 : x3::CfgS1::W2);
        const int lds = alt  ? x3::MidPlan<x3::CfgS2Alt::C / 2, x3::CfgS2Alt::W2>::LDS_BYTES
                        : s2 ? x3::MidPlan<x3::CfgS2::C / 2, x3::CfgS2::W2>::LDS_BYTES
                             : x3::MidPlan<x3::CfgS1::C / 2, x3::CfgS1::W2>::LDS_BYTES;
        p.mid_g = {cdiv(4 * T, p.mid_w), B, (s2 ? x3::CfgS2::MW : x3::CfgS1::MW) * 64, lds};
    }
    return p;
}

inline int VocLaunchPlan::print(char* out, size_t cap) const {
    size_t n = 0;
    auto put = [&](const char* fmt, auto... a) {
        const int k = std::snprintf(out && n < cap ? out + n : nullptr, out && n < cap ? cap - n : 0, fmt, a...);
        if (k > 0) n += (size_t)k;
    };
    auto grid = [&](const VocGrid& g) { put(" grid=%dx%d thr=%d lds=%d]", g.x, g.y, g.threads, g.lds); };
    if (path == VocPath::PerLayer) {
        put("%s", "perlayer");
        return (int)n;
    }
    const f32::FormRow& f = f32::kF32Forms[form];
    if (path == VocPath::F32) {
        put("f32 stage=%d form=%s pair=%d comp=%d trans=%d head[tf=%d", stage, f.name, (int)pair, (int)f32_comp, (int)trans,
            f32::kTiling[f.head].tf);
        grid(head_g);
        put(" mid[w=%d", f32::kTiling[f.mid].w2);
        grid(mid_g);
        put(" tail[w=%d", f32::kTiling[f.tail].w3);
        grid(tail_g);
        put("%s", " redo=none");
        return (int)n;
    }
    put("split stage=%d ", stage);
    if (headmid) {
        put("headmid[n=%d S=%d nch=%d trans=%d", hm_n, hm_S, hm_nch, (int)trans);
        grid(head_g);
    } else {
        put("head[tf=%d comp=%d trans=%d", head_tf, (int)comp, (int)trans);
        grid(head_g);
        if (mid == VocMid::Midp) put(" midp[nch=%d", mid_nch);
        else put(" x3mid[alt=%d w=%d", (int)(mid == VocMid::X3Alt), mid_w);
        grid(mid_g);
    }
    if (tail == VocTail::Tailp || tail == VocTail::Tailp2)
        put(" %s[nl=%d nch=%d", tail == VocTail::Tailp ? "tailp" : "tailp2", tail_nl, tail_nch);
    else put(" x3tail[alt=%d w=%d", (int)(tail == VocTail::X3Alt), tail_w);
    grid(tail_g);
    if (redo == VocRedoPlan::Guarded)
        put(" redo=guarded[%s pair=%d comp=%d thr=%d lds=%d]", f32::kTiling[f.redo].name, (int)pair, (int)f32_comp,
            redo_g.threads, redo_g.lds);
    else put(" redo=%s", redo == VocRedoPlan::None ? "none" : redo == VocRedoPlan::InTail ? "in-tail" : "host");
    if (no_headmid) put(" no-headmid=\"%s\"", no_headmid);
    return (int)n;
}

}  // namespace m2
