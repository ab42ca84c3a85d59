// What the pipelined split-f16 vocoder kernels share (vocoder_midp.hip,
// vocoder_tailp.hip, vocoder_tailp2.hip): the device helpers of a pipeline
// role, the host packers that cut a dense polyphase matrix into MFMA weight
// fragments, the composed output layer.  (The strip-length choice is part of the launch plan:
// pipe::pick_strip, vocoder_launch.h.)  Slot
// tables, ring layouts and the roles themselves belong to each kernel.
#pragma once
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "m2_common.h"
#include "vocoder_fused.h"

namespace m2 {
namespace pipe {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef vx_u32x4 u32x4;
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int V>
using ic = std::integral_constant<int, V>;

__device__ __forceinline__ f32x4 mfma_h(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
}

// LDS hand-off between roles: the step's ds_writes complete, then the
// workgroup barrier.  No vmcnt wait (the loader's prefetches stay in flight),
// and the "memory" clobber keeps the compiler from moving LDS accesses across.
// (An LDS-flag protocol that lets the roles run decoupled measured slower:
// 48 vs 35.5 us, its polls sit on every hand-off of the chain.)
__device__ __forceinline__ void step_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// tanh(x) = 1 - 2 / (1 + e^{2x}) on v_exp_f32 / v_rcp_f32: absolute error
// ~1e-7 (saturates to +-1 through inf / 0), against ~40 instructions for tanhf.
__device__ __forceinline__ float tanh_fast(float x) { return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __expf(2.f * x)); }

// Layer l computes chunk k in step k + l + 1; the last step is the last
// layer's chunk nch - 1, nl the number of computing layers.  (Staggered
// epilogues, where some layers store chunk k one step after computing it,
// measured slower and were dropped.)
constexpr int off_l(int l) { return l + 1; }
constexpr int last_step(int nch, int nl) { return nch - 1 + off_l(nl - 1); }

// Row of column offset c (-2 .. 16) of the chunk in ring phase j of an R-row ring.
__device__ __forceinline__ int ring_row(int R, int j, int c) {
    const int r = 16 * j + c;
    return r < 0 ? r + R : (r >= R ? r - R : r);
}

// ---------------------------------------------------------------------------
// Host packing.  A layer is first written as a dense polyphase matrix
// Wd[row][dq + 1][input row] over the columns q of the kernel's input, then
// cut into (m-block, k-block) weight units along the kernel's slot table.

constexpr int floordiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

template <typename T>
struct PolyDenseT {
    int rows, width;
    std::vector<T> w;
    PolyDenseT(int rows_, int width_) : rows(rows_), width(width_), w((size_t)rows_ * 3 * width_, T(0)) {}
    T& at(int row, int dq, int in) { return w[((size_t)row * 3 + dq + 1) * width + in]; }
    T at(int row, int dq, int in) const { return w[((size_t)row * 3 + dq + 1) * width + in]; }
};
using PolyDense = PolyDenseT<float>;

// ConvTranspose1d(k=4, stride 2, pad 1), W [Cin][Cout][4], on a Pin-phase input
// (Cin channels per phase) -> 2*Pin phases of Cout channels (tts_model.py:255-263):
// out[2i] = x[i] W1 + x[i-1] W3, out[2i+1] = x[i+1] W0 + x[i] W2.
inline void dense_convT2(PolyDense& d, const float* W, int Pin, int Cin, int Cout) {
    const int taps[2][2][2] = {{{0, 1}, {-1, 3}}, {{1, 0}, {0, 2}}};  // [s][j] = (input offset, kernel tap)
    for (int pin = 0; pin < Pin; ++pin)
        for (int s = 0; s < 2; ++s)
            for (int j = 0; j < 2; ++j) {
                const int pp = pin + taps[s][j][0], dq = floordiv(pp, Pin), p2 = pp - dq * Pin, kk = taps[s][j][1];
                for (int co = 0; co < Cout; ++co)
                    for (int ci = 0; ci < Cin; ++ci)
                        d.at((2 * pin + s) * Cout + co, dq, p2 * Cin + ci) += W[((size_t)ci * Cout + co) * 4 + kk];
            }
}

// Conv1d(k=3, pad 1), W [Cout][Cin][3], on a P-phase signal: tap t + k - 1 of
// phase p is phase (p + k - 1) mod P of column q + floor((p + k - 1) / P).
inline void dense_conv3(PolyDense& d, const float* W, int P, int Cin, int Cout) {
    for (int p = 0; p < P; ++p)
        for (int k = 0; k < 3; ++k) {
            const int pp = p + k - 1, dq = floordiv(pp, P), p2 = pp - dq * P;
            for (int co = 0; co < Cout; ++co)
                for (int ci = 0; ci < Cin; ++ci) d.at(p * Cout + co, dq, p2 * Cin + ci) += W[((size_t)co * Cin + ci) * 3 + k];
        }
}

// One weight as its unscaled (hi, lo) f16 pair (split2u's format): hi at idx,
// lo one 64-lane x 8-element fragment later.
inline void put_split(std::vector<uint16_t>& out, size_t idx, float v, bool* range_ok) {
    if (!(std::fabs(v) < 65504.f)) *range_ok = false;
    const _Float16 h = (_Float16)v;
    const _Float16 l = (_Float16)(v - (float)h);
    uint16_t hb, lb;
    std::memcpy(&hb, &h, 2);
    std::memcpy(&lb, &l, 2);
    out[idx] = hb;
    out[idx + 64 * 8] = lb;
}

// One m-block's weight units unit0 .. unit0 + nkb - 1 of *wout (sized by the
// caller), one per k-block: A[lane row li][slot g = lane >> 4, element e] =
// d[row(li)][dq][8 oct + e] with (dq, oct) = slot(kb, g), zero for a row past
// the matrix and on a slot the m-block already reads in an earlier (kb, g).
// False when a non-zero of the m-block's rows sits on none of its slots.
template <typename T, typename RowFn, typename SlotFn>
bool cut_fragments(const PolyDenseT<T>& d, int unit0, int nkb, RowFn row, SlotFn slot, std::vector<uint16_t>* wout,
                   bool* range_ok) {
    auto same = [](auto a, auto b) { return a.dq == b.dq && a.oct == b.oct; };
    for (int li = 0; li < 16; ++li) {
        if (row(li) >= d.rows) continue;
        for (int dq = -1; dq <= 1; ++dq)
            for (int in = 0; in < d.width; ++in) {
                if (d.at(row(li), dq, in) == T(0)) continue;
                bool found = false;
                for (int j = 0; j < 4 * nkb && !found; ++j) {
                    const auto sl = slot(j / 4, j % 4);
                    found = sl.dq == dq && sl.oct == in / 8;
                }
                if (!found) return false;
            }
    }
    for (int kb = 0; kb < nkb; ++kb)
        for (int lane = 0; lane < 64; ++lane) {
            const int r = row(lane & 15), g = lane >> 4;
            const auto sl = slot(kb, g);
            bool dup = false;
            for (int j = 0; j < kb * 4 + g; ++j) dup = dup || same(slot(j / 4, j % 4), sl);
            for (int e = 0; e < 8; ++e) {
                const T v = r < d.rows && !dup ? d.at(r, sl.dq, 8 * sl.oct + e) : T(0);
                put_split(*wout, (((size_t)(unit0 + kb) * 2) * 64 + lane) * 8 + e, (float)v, range_ok);
            }
        }
    return true;
}

// ResBlock4 conv2 and output_conv composed into one layer (the tails'
// six-layer form), in double, at C channels (8 or 16): the resblock's output
// y = conv2(h) + b2 + x feeds only the linear output conv, so
// audio[t] = tanh(bo' + sum_d Wo[c][d] x[c][t+d] + sum_j Wc[c'][j] h[c'][t+j]),
// Wc[c'][j] = sum_{d+e=j} sum_c Wo[c][d] W2[c][c'][e], bo' = bo + sum_d sum_c
// Wo[c][d] b2[c]; on the 4-phase columns (row p = output phase, input row
// p2 * C + c at column q + dq).  Weight units unit0 .. + nfh - 1 read h
// (ResBlock4's intermediate), the next nfx read x (ConvT4's output); fragment
// f's lane group g reads slot(f, g).  bout gets bo' (rows 0..3) at bias_at and
// the edge terms at corr_at: the y the composed form sees at t = -1 is
// b2 + W2[.][.][2] h[., 0], at t = L4 it is b2 + W2[.][.][0] h[., L4-1], so
// vL[C], vR[C], kL, kR with v = Wo o W2 on that tap and k = Wo . b2.
template <typename SlotFn>
bool pack_outc_layer(const TailpSrc& s, int C, int unit0, int nfh, int nfx, SlotFn slot, int bias_at, int corr_at,
                     std::vector<uint16_t>* wout, std::vector<float>* bout, bool* range_ok) {
    PolyDenseT<double> dh(4, 4 * C), dx(4, 4 * C);
    auto wo = [&](int c, int k) { return (double)s.wo[c * 3 + k]; };
    auto w2 = [&](int c, int ci, int k) { return (double)s.w42[(c * C + ci) * 3 + k]; };
    for (int p = 0; p < 4; ++p)
        for (int d = -1; d <= 1; ++d)
            for (int c = 0; c < C; ++c) {
                const int tx = p + d, qx = floordiv(tx, 4);
                dx.at(p, qx, (tx - 4 * qx) * C + c) += wo(c, d + 1);
                for (int e = -1; e <= 1; ++e)
                    for (int ci = 0; ci < C; ++ci) {
                        const int th = p + d + e, qh = floordiv(th, 4);
                        dh.at(p, qh, (th - 4 * qh) * C + ci) += wo(c, d + 1) * w2(c, ci, e + 1);
                    }
            }
    auto row = [](int li) { return li; };
    if (!cut_fragments(dh, unit0, nfh, row, slot, wout, range_ok)) return false;
    if (!cut_fragments(dx, unit0 + nfh, nfx, row, [&](int kb, int g) { return slot(nfh + kb, g); }, wout, range_ok))
        return false;
    double bo = s.bo[0], kl = 0.0, kr = 0.0;
    for (int c = 0; c < C; ++c) {
        for (int k = 0; k < 3; ++k) bo += wo(c, k) * s.b42[c];
        kl += wo(c, 0) * s.b42[c];
        kr += wo(c, 2) * s.b42[c];
    }
    for (int r = 0; r < 4; ++r) (*bout)[bias_at + r] = (float)bo;
    for (int ci = 0; ci < C; ++ci) {
        double vl = 0.0, vr = 0.0;
        for (int c = 0; c < C; ++c) {
            vl += wo(c, 0) * w2(c, ci, 2);
            vr += wo(c, 2) * w2(c, ci, 0);
        }
        (*bout)[corr_at + ci] = (float)vl;
        (*bout)[corr_at + C + ci] = (float)vr;
    }
    (*bout)[corr_at + 2 * C] = (float)kl;
    (*bout)[corr_at + 2 * C + 1] = (float)kr;
    return true;
}

}  // namespace pipe
}  // namespace m2
