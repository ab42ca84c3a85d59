// The host-only half of duration_grad.hip: the tape of DurationPredictor's training forward, the
// workspace of its backward and every launch of one m2_duration_backward call.  Pure arithmetic on the
// host, as encoder_grad_plan.h: tools/plan_check.cpp runs all of it on the CPU.
//
// The function, for enc [B, S, H] read as x = enc^T [B, H, S]:
//   u1 = conv1(x) + b1 (k = 3, padding 1),   y1 = relu(u1 alpha1 + beta1'),
//   u2 = conv2(y1) + b2,                     y2 = relu(u2 alpha2 + beta2'),
//   z = proj(y2) + pb (k = 1, H -> 1),       dur = softplus(z) (beta 1, threshold 20).
// alpha = gamma / sqrt(running_var + eps) and beta' = beta - running_mean alpha: running statistics as
// constants (eval-mode BatchNorm), no dropout.  Parameters in parameters() order (P_*): (conv.weight
// [H, H, 3], conv.bias, norm.weight, norm.bias) x 2, projection.weight [1, H, 1], projection.bias.  `bn`
// is 8 vectors [H], block-major (BN_*): alpha, beta', running_mean and invstd = 1 / sqrt(running_var +
// eps) of block 1, then of block 2; the forward reads alpha and beta', the backward alpha, mean and invstd.
//
// The tape: y1 and y2 [B, H, S], post-ReLU, each on a 256-byte boundary (m2_duration_tape_map's index 0
// and 1): the ReLU's predicate is the stored value > 0.  u is NOT on the tape: d gamma needs u itself
// (gamma may be 0 or negative, so u cannot be had from y), and the backward recomputes it with the
// forward's own conv launch without affine and activation (steps u2, u1), the bits the fused forward
// held in registers.  z is recomputed by the head kernel in the forward's order (fmaf over the channels
// ascending, then the bias).  x = enc^T is not on the tape either: the backward transposes enc into the
// workspace (step xt) for the recomputation of u1 and conv1's weight gradient.
//
// The workspace: xt, u, gu, gy, each [B, H, S]; the partials of the widest reduction (`part`); one conv
// weight and one bias (`wtmp`, `btmp`): with `accumulate` a conv's weight and bias gradient are formed
// there as without it and added onto the caller's tensor by a one-slot dec_finish_kernel, one fp32
// addition per element (the slot reductions add their sum onto the caller's tensor directly).
//
// The steps of one call (plan_steps), every gradient and d_enc asked for:
//   xt  dur_transpose_kernel   enc [B, S, H] -> xt [B, H, S]
//   u2  conv_kernel            u = conv2(y1) + b2
//   hd  dur_bn_bwd_kernel      the head: g_z from d_dur and z, g_y2 = pw g_z, g_a = g_y2 [y2 > 0],
//                              gu = g_a alpha2; slots of d gamma2, d beta2, d pw, d pb; four finishes
//   c2  launch_conv_bwd        gy = conv2's data gradient of gu; its weight and bias gradients
//   u1  conv_kernel            u = conv1(xt) + b1
//   b1  dur_bn_bwd_kernel      gu = gy [y1 > 0] alpha1; slots of d gamma1, d beta1; two finishes
//   c1  launch_conv_bwd        gy = conv1's data gradient of gu; its weight and bias gradients
//   dt  dur_transpose_kernel   gy [B, H, S] -> d_enc [B, S, H]
// xt, u2, u1, b1, c2's and c1's parts and dt are skipped when nobody asked for what they feed; the head
// always runs and writes all its slots, of which only the wanted ones are finished.  The conv launchers
// take int dimensions: dims_ok keeps a map (B H S) within 2^30 floats.  Every reduction over (utterance, position) goes
// through per-workgroup slots (one per utterance and 64-position chunk) added in a fixed order; d_enc
// has no reduction over the batch.
//
// The printed form (m2_debug_duration_grad_plan) is the other gradient plans', one line:
//   H= B= S= tape=<bytes> ws=<bytes> part=<floats> u=recomputed
// then one item per launch, <step>:<kernel>[grid=<x>x<y>x<z> thr=<threads> lds=<bytes>].
#pragma once

#include <cstdio>
#include <string>
#include <vector>

#include "layer_grad_plan.h"

namespace m2 {
namespace dugrad {

using loss::ConvGeo;
using loss::LaunchRow;

constexpr int kParams = 10;
constexpr int kMaps = 2;
constexpr int kBn = 8;
constexpr int kChunk = 64;    // positions per dur_bn_bwd_kernel workgroup, one per lane
constexpr int kTile = 32;     // dur_transpose_kernel: a 32 x 32 tile at a pitch of 33 floats
constexpr int kConvCo = 8;    // conv_kernel (vocoder.hip): output channels per workgroup when Cout % 8 == 0
constexpr int kConvPos = 1024;  // and positions per workgroup (256 threads x 4)

enum Param { P_W1 = 0, P_B1 = 1, P_G1 = 2, P_BE1 = 3, P_W2 = 4, P_B2 = 5, P_G2 = 6, P_BE2 = 7, P_PW = 8, P_PB = 9 };
enum Bn { BN_ALPHA = 0, BN_BETA = 1, BN_MEAN = 2, BN_INVSTD = 3 };  // + 4 block
enum Map { MAP_Y1 = 0, MAP_Y2 = 1 };

struct Dims {
    int H, B, S;
};
inline bool dims_ok(const Dims& d) {
    return d.H >= 16 && d.H <= 128 && d.H % 8 == 0 && d.B >= 0 && d.B <= loss::kMaxGrid && d.S >= 0 &&
           d.S <= (1 << 20) && (long long)d.B * d.S <= (1 << 24) && (long long)d.B * d.H * d.S <= (1 << 30);
}
inline size_t map_floats(const Dims& d) { return (size_t)d.B * d.H * d.S; }
inline ConvGeo geo(const Dims& d) { return ConvGeo{d.H, d.H, 3, 1, 1, 1}; }

// The one statement of the tape: over a Sizer the byte count, over a Carve the maps.
template <typename A>
void carve_tape(A& a, const Dims& d, float* maps[kMaps]) {
    for (int i = 0; i < kMaps; ++i) {
        float* p = a.template take<float>(map_floats(d));
        if (maps) maps[i] = p;
    }
}

// ---- the kernels' geometry ---------------------------------------------------------

inline int chunks(int S) { return cdiv(S, kChunk); }
inline size_t slots(const Dims& d) { return (size_t)d.B * chunks(d.S); }
// Floats of one workgroup's slot: d gamma [H], d beta [H], and for the head d pw [H], d pb.
inline size_t slot_floats(int H, bool head) { return head ? 3 * (size_t)H + 1 : 2 * (size_t)H; }
inline LaunchRow bn_row(const Dims& d, bool head) {
    return {"dur_bn_bwd_kernel", (unsigned)chunks(d.S), (unsigned)d.B, 1, 256,
            head ? (size_t)d.H * kChunk * sizeof(float) : 0};
}
// in [B, R, C] -> out [B, C, R]
inline LaunchRow tr_row(int B, int R, int C) {
    return {"dur_transpose_kernel", (unsigned)cdiv(C, kTile), (unsigned)cdiv(R, kTile), (unsigned)B, 256, 0};
}
inline LaunchRow conv_fwd_row(const Dims& d) {
    return {"conv_kernel", (unsigned)cdiv(d.S, kConvPos), (unsigned)(d.H / kConvCo), (unsigned)d.B, 256, 0};
}
using dgrad::finish_row;  // dec_finish_kernel over n elements

// ---- the steps of one backward call ------------------------------------------------

enum StepKind { STEP_XT = 0, STEP_U = 1, STEP_HEAD = 2, STEP_BN = 3, STEP_CONV = 4, STEP_DT = 5 };
struct Step {
    StepKind kind;
    char label[4];
    int block;  // 0 or 1: the ConvBlock of the step (STEP_U, STEP_BN, STEP_CONV, STEP_HEAD: 1); else -1
};
inline std::vector<Step> plan_steps(const Dims&) {
    return {{STEP_XT, "xt", -1}, {STEP_U, "u2", 1},    {STEP_HEAD, "hd", 1}, {STEP_CONV, "c2", 1},
            {STEP_U, "u1", 0},   {STEP_BN, "b1", 0},   {STEP_CONV, "c1", 0}, {STEP_DT, "dt", -1}};
}

// The launches of one step with every gradient and d_enc asked for; `accumulate`: the one-slot finishes
// that add a conv's weight and bias gradient onto the caller's tensors.
inline void step_rows(const Step& s, const Dims& d, bool accumulate, std::vector<LaunchRow>& out) {
    const size_t H = (size_t)d.H;
    switch (s.kind) {
        case STEP_XT: out.push_back(tr_row(d.B, d.S, d.H)); break;
        case STEP_U: out.push_back(conv_fwd_row(d)); break;
        case STEP_HEAD:
            out.push_back(bn_row(d, true));
            for (const size_t n : {H, H, H, (size_t)1}) out.push_back(finish_row(n));
            break;
        case STEP_BN:
            out.push_back(bn_row(d, false));
            for (const size_t n : {H, H}) out.push_back(finish_row(n));
            break;
        case STEP_CONV:
            loss::conv_bwd_rows(geo(d), d.B, d.S, true, true, true, out);
            if (accumulate) {
                out.push_back(finish_row(3 * H * H));
                out.push_back(finish_row(H));
            }
            break;
        case STEP_DT: out.push_back(tr_row(d.B, d.H, d.S)); break;
    }
}

inline size_t part_floats(const Dims& d) {
    return std::max(slots(d) * slot_floats(d.H, true), loss::dw_plan(geo(d), d.B, d.S).part_floats);
}

struct Bufs {
    float* xt;
    float* u;
    float* gu;
    float* gy;
    float* part;
    float* wtmp;
    float* btmp;
};

// The one statement of the backward's workspace.
template <typename A>
void carve_backward(A& a, const Dims& d, Bufs* out) {
    Bufs b{};
    const size_t n = map_floats(d);
    b.xt = a.template take<float>(n);
    b.u = a.template take<float>(n);
    b.gu = a.template take<float>(n);
    b.gy = a.template take<float>(n);
    b.part = a.template take<float>(part_floats(d));
    b.wtmp = a.template take<float>((size_t)3 * d.H * d.H);
    b.btmp = a.template take<float>((size_t)d.H);
    if (out) *out = b;
}

inline std::string print_plan(const Dims& d) {
    Sizer t, w;
    carve_tape(t, d, nullptr);
    carve_backward(w, d, nullptr);
    char buf[256];
    std::snprintf(buf, sizeof(buf), "H=%d B=%d S=%d tape=%zu ws=%zu part=%zu u=recomputed", d.H, d.B, d.S, t.off + 256,
                  w.off + 256, part_floats(d));
    std::string line(buf);
    for (const Step& s : plan_steps(d)) {
        std::vector<LaunchRow> rows;
        step_rows(s, d, false, rows);
        for (const LaunchRow& r : rows) {
            std::snprintf(buf, sizeof(buf), " %s:%s[grid=%ux%ux%u thr=%d lds=%zu]", s.label, r.kernel, r.gx, r.gy, r.gz,
                          r.threads, r.lds);
            line += buf;
        }
    }
    return line;
}

}  // namespace dugrad
}  // namespace m2
