// The host-only half of vocoder_grad.hip: the tape of the training forward, the workspace of
// the backward and every launch of one m2_vocoder_backward call.  Pure arithmetic on the host:
// nothing here touches a device, so tools/plan_check.cpp runs all of it on the CPU.  Both _bytes
// queries run the carves over a Sizer and both calls run them over a Carve before anything is
// launched; m2_vocoder_backward walks plan_steps() and launches what each step's rows name.
//
// The tape, stated once.  Maps are float32 [B, channels, length], each on a 256-byte boundary, in
// this order (m2_vocoder_tape_map's index); c_k = C / 2^(k+1), L_k = T x 4, 16, 32, 64:
//    0           h      [C, T]       input_conv(mel)
//    1 + 3k      a_k    [c_k, L_k]   leaky(ConvT_k(x_k)): the stored value is post-activation
//    2 + 3k      lv_k   [c_k, L_k]   leaky(conv1_k(a_k)): post-activation
//    3 + 3k      x_k+1  [c_k, L_k]   conv2_k(lv_k) + a_k
//   13           y      [1, 64 T]    the audio, for tanh' = 1 - y^2
// Slope 0.1 keeps the sign, so leaky' reads its predicate (value > 0) from the stored value.
//
// The workspace: the cotangent of a stage's output (cot[0]: g_r, then g_x below the ConvT) and of
// the ConvT's output (cot[1]: g_u), g_v, each B x the widest map, the partials of the widest
// reduction (`part`), and one weight and one bias of the largest size (`wtmp`, `btmp`): with
// `accumulate` every gradient is formed there as without it and then added onto the caller's
// tensor by voc_add_kernel, one fp32 addition per element whatever kernel formed it.
//
// The printed form (m2_debug_vocoder_grad_plan) is one line of space-separated items, fixed:
//   M= C= B= T= tape=<bytes> ws=<bytes> cot=<floats> part=<floats>
// then one item per launch, in launch order,
//   <step>:<kernel>[grid=<x>x<y>x<z> thr=<threads> lds=<bytes>]
// <step> is out | res<k> | c2w<k> | c1w<k> | upb<k> | upw<k> | updx<k> | in (k = 3..0): the output
// conv, the resblock's data gradient, the weight and bias gradients of conv2, conv1 and the
// ConvT's bias and weight, the ConvT's data gradient, the input conv.  The line is that of a call
// with every gradient and d_mel asked for and `accumulate` off (with it on, one voc_add_kernel
// launch follows each gradient).
#pragma once

#include <cstdio>
#include <string>
#include <vector>

#include "losses_plan.h"

namespace m2 {
namespace vgrad {

using loss::ConvGeo;
using loss::LaunchRow;

constexpr int kStages = 4;
constexpr int kRates[kStages] = {4, 4, 2, 2};
constexpr int kParams = 28;  // state_dict order: input_conv, upsamples.k, resblocks.k.conv1 / conv2, output_conv
constexpr int kMaps = 14;
constexpr int kMaxC = 256;   // voc_res_dx_kernel stages two windows of c <= 128 channels

constexpr int kOutP = 1024;  // positions per voc_out_bwd workgroup (4 per thread)
constexpr int kNwP = 256;    // output positions per voc_dw_narrow chunk
constexpr int kNwSplits = 512;  // partials of one narrow weight gradient, at most

inline int p_in() { return 0; }
inline int p_up(int k) { return 2 + 2 * k; }
inline int p_c1(int k) { return 10 + 4 * k; }
inline int p_c2(int k) { return 12 + 4 * k; }
inline int p_out() { return 26; }

struct Dims {
    int M, C, B, T;
};
inline bool dims_ok(const Dims& d) {
    return d.M >= 1 && d.M <= loss::kMaxGrid && d.C >= 16 && d.C % 16 == 0 && d.C <= kMaxC && d.B >= 0 &&
           d.B <= loss::kMaxGrid && d.T >= 0 && d.T <= (1 << 22) && (long long)d.B * d.T <= (1 << 24);
}
inline int stage_c(const Dims& d, int k) { return d.C >> (k + 1); }
inline int stage_len(const Dims& d, int k) {
    int L = d.T;
    for (int i = 0; i <= k; ++i) L *= kRates[i];
    return L;
}

enum Map { MAP_H = 0, MAP_Y = 13 };
inline int map_a(int k) { return 1 + 3 * k; }
inline int map_lv(int k) { return 2 + 3 * k; }
inline int map_x(int k) { return k == 0 ? (int)MAP_H : 3 * k; }  // x_k, the input of stage k

inline void map_shape(const Dims& d, int index, int* channels, int* length) {
    if (index == MAP_H) {
        *channels = d.C;
        *length = d.T;
    } else if (index == MAP_Y) {
        *channels = 1;
        *length = 64 * d.T;
    } else {
        const int k = (index - 1) / 3;
        *channels = stage_c(d, k);
        *length = stage_len(d, k);
    }
}

// The one statement of the tape: over a Sizer the byte count, over a Carve the maps.
template <typename A>
void carve_tape(A& a, const Dims& d, float* maps[kMaps]) {
    for (int i = 0; i < kMaps; ++i) {
        int c, n;
        map_shape(d, i, &c, &n);
        float* p = a.template take<float>((size_t)d.B * c * n);
        if (maps) maps[i] = p;
    }
}

// ---- the three kernels' geometry ---------------------------------------------------

// voc_res_dx_kernel: the width of g_v's window (a power of two; the workgroup's own positions are
// two fewer), the widest whose windows of g_r (W + 2) and g_v (W) over c channels fit LDS.
inline int res_width(int c) {
    for (int W = 256; W >= 32; W >>= 1)
        if ((size_t)c * (2 * W + 2) * sizeof(float) <= (size_t)loss::kMaxLds) return W;
    return 0;
}
inline size_t res_lds_bytes(int c) { return (size_t)c * (2 * res_width(c) + 2) * sizeof(float); }
inline LaunchRow res_row(int c, int nb, int L) {
    return {"voc_res_dx_kernel", (unsigned)cdiv(L, res_width(c) - 2), (unsigned)nb, 1, 256, res_lds_bytes(c)};
}

// voc_out_bwd_kernel: partial slots [nb x chunks], 3 c floats of dw and one of db each.
inline int out_chunks(int L) { return cdiv(L, kOutP); }
inline size_t out_part_floats(int c, int nb, int L) { return (size_t)nb * out_chunks(L) * (3 * (size_t)c + 1); }
inline LaunchRow out_row(int nb, int L) {
    return {"voc_out_bwd_kernel", (unsigned)out_chunks(L), (unsigned)nb, 1, 256, (kOutP + 2) * sizeof(float)};
}

// voc_dw_narrow_kernel: the weight (and bias) partials of a Conv1d with fewer than 16 output channels.
struct NarrowPlan {
    bool ok = false;
    int splits = 0, cps = 0;
    size_t lds = 0, part_floats = 0;
};
inline NarrowPlan narrow_plan(const ConvGeo& g, int nb, int L) {
    NarrowPlan p;
    const int Lo = loss::conv_out_len(L, g);
    if (g.groups != 1 || g.Cout >= 16 || g.Cout < 1 || g.Cin < 1 || Lo < 1 || g.stride > 64 || g.k > 256) return p;
    const size_t n = (size_t)g.Cout * g.Cin * g.k, span = (size_t)(kNwP - 1) * g.stride + g.k;
    p.lds = ((size_t)g.Cout * kNwP + (size_t)g.Cin * span + n + g.Cout) * sizeof(float);
    const long long chunks = (long long)nb * cdiv(Lo, kNwP);
    if (p.lds > (size_t)loss::kMaxLds || chunks > (1 << 30) || chunks < 1) return p;
    p.ok = true;
    p.splits = (int)std::min<long long>(chunks, kNwSplits);
    p.cps = (int)((chunks + p.splits - 1) / p.splits);
    p.splits = (int)((chunks + p.cps - 1) / p.cps);
    p.part_floats = (size_t)p.splits * (n + g.Cout);
    return p;
}
inline void narrow_rows(const ConvGeo& g, int nb, int L, bool dw, bool db, std::vector<LaunchRow>& out) {
    const NarrowPlan p = narrow_plan(g, nb, L);
    const size_t n = (size_t)g.Cout * g.Cin * g.k;
    out.push_back({"voc_dw_narrow_kernel", (unsigned)p.splits, 1, 1, 256, p.lds});
    if (dw) out.push_back({"dw_finish_kernel", (unsigned)((n + 255) / 256), 1, 1, 256, 0});
    if (db) out.push_back({"dw_finish_kernel", (unsigned)cdiv(g.Cout, 256), 1, 1, 256, 0});
}

// ---- the steps of one backward call ------------------------------------------------

enum StepKind {
    STEP_OUT = 0,     // voc_out_bwd_kernel and its two finishes
    STEP_RES = 1,     // voc_res_dx_kernel
    STEP_WGRAD = 2,   // weight and bias gradients of a Conv1d, no data gradient: launch_conv_bwd on the MFMA,
                      // voc_dw_narrow_kernel below 16 output channels
    STEP_BIAS = 3,    // conv_db_kernel
    STEP_CONV = 4,    // launch_conv: the ConvT's data gradient as a strided Conv1d
    STEP_IN = 5       // launch_conv_bwd with the data gradient: the input conv
};
// Buffers a step reads and writes: a tape map (0..13) or one of these.
enum Buf { BUF_NONE = -1, BUF_COT0 = 16, BUF_COT1 = 17, BUF_GV = 18, BUF_MEL = 19, BUF_DAUDIO = 20, BUF_DMEL = 21 };

struct Step {
    StepKind kind;
    char label[8];
    int stage;     // k, or -1 (the output and input convs)
    ConvGeo g;     // the Conv1d of the step (STEP_RES, STEP_OUT: Cin = Cout = c)
    int L;         // its input length
    int x, dy;     // the layer's input and its output's cotangent
    int w, dw, db; // parameter indices: the weight read, the gradients written (-1: none)
    bool narrow;   // STEP_WGRAD through voc_dw_narrow_kernel
};

inline Step make_step(StepKind kind, const char* name, int k, const ConvGeo& g, int L, int x, int dy, int w, int dw,
                      int db) {
    Step s{};
    s.kind = kind;
    s.stage = k;
    if (k >= 0) std::snprintf(s.label, sizeof(s.label), "%s%d", name, k);
    else std::snprintf(s.label, sizeof(s.label), "%s", name);
    s.g = g;
    s.L = L;
    s.x = x;
    s.dy = dy;
    s.w = w;
    s.dw = dw;
    s.db = db;
    s.narrow = false;
    return s;
}

// A weight-gradient step takes the narrow kernel where dw_plan leaves the MFMA and the narrow plan fits.
inline Step wgrad_step(const char* name, int k, const ConvGeo& g, int nb, int L, int x, int dy, int dw, int db) {
    Step s = make_step(STEP_WGRAD, name, k, g, L, x, dy, -1, dw, db);
    s.narrow = !loss::dw_plan(g, nb, L).mfma && narrow_plan(g, nb, L).ok;
    return s;
}

// The ConvTranspose1d of stage k read as the Conv1d its gradients are: Cin' = c_k, Cout' = c_(k-1),
// kernel 2 r, stride r, padding r / 2 over the ConvT's output length.
inline ConvGeo convT_as_conv(const Dims& d, int k) {
    const int r = kRates[k];
    return ConvGeo{stage_c(d, k), d.C >> k, 2 * r, r, r / 2, 1};
}

inline std::vector<Step> plan_steps(const Dims& d) {
    std::vector<Step> s;
    const int c3 = stage_c(d, 3), L3 = stage_len(d, 3);
    s.push_back(make_step(STEP_OUT, "out", -1, ConvGeo{c3, 1, 3, 1, 1, 1}, L3, 3 * kStages, BUF_DAUDIO, p_out(), p_out(),
                          p_out() + 1));
    for (int k = kStages - 1; k >= 0; --k) {
        const int c = stage_c(d, k), L = stage_len(d, k);
        const ConvGeo g{c, c, 3, 1, 1, 1};
        s.push_back(make_step(STEP_RES, "res", k, g, L, BUF_NONE, BUF_COT0, -1, -1, -1));
        s.push_back(wgrad_step("c2w", k, g, d.B, L, map_lv(k), BUF_COT0, p_c2(k), p_c2(k) + 1));
        s.push_back(wgrad_step("c1w", k, g, d.B, L, map_a(k), BUF_GV, p_c1(k), p_c1(k) + 1));
        const ConvGeo gt = convT_as_conv(d, k);
        s.push_back(make_step(STEP_BIAS, "upb", k, gt, L, BUF_NONE, BUF_COT1, -1, -1, p_up(k) + 1));
        s.push_back(wgrad_step("upw", k, gt, d.B, L, BUF_COT1, map_x(k), p_up(k), -1));
        s.push_back(make_step(STEP_CONV, "updx", k, gt, L, BUF_COT1, BUF_COT0, p_up(k), -1, -1));
    }
    s.push_back(make_step(STEP_IN, "in", -1, ConvGeo{d.M, d.C, 3, 1, 1, 1}, d.T, BUF_MEL, BUF_COT0, p_in(), p_in(),
                          p_in() + 1));
    return s;
}

// The launches of one step over nb utterances; dx, dw, db: which of its outputs are asked for.
inline void step_rows(const Step& s, int nb, bool dx, bool dw, bool db, std::vector<LaunchRow>& out) {
    switch (s.kind) {
        case STEP_OUT:
            out.push_back(out_row(nb, s.L));
            if (dw) out.push_back({"dw_finish_kernel", (unsigned)cdiv(3 * s.g.Cin, 256), 1, 1, 256, 0});
            if (db) out.push_back({"dw_finish_kernel", 1, 1, 1, 256, 0});
            break;
        case STEP_RES: out.push_back(res_row(s.g.Cin, nb, s.L)); break;
        case STEP_WGRAD:
            if (!dw && !db) break;
            if (s.narrow) narrow_rows(s.g, nb, s.L, dw, db, out);
            else loss::conv_bwd_rows(s.g, nb, s.L, false, dw, db, out);
            break;
        case STEP_BIAS:
            if (db) out.push_back({"conv_db_kernel", (unsigned)s.g.Cin, 1, 1, loss::kDbThreads, 0});
            break;
        case STEP_CONV: out.push_back(loss::conv_row(s.g, nb, s.L)); break;
        case STEP_IN:
            if (dx || dw || db) loss::conv_bwd_rows(s.g, nb, s.L, dx, dw, db, out);
            break;
    }
}

// Floats of partials a step needs in the workspace.
inline size_t step_part_floats(const Step& s, int nb) {
    switch (s.kind) {
        case STEP_OUT: return out_part_floats(s.g.Cin, nb, s.L);
        case STEP_WGRAD:
        case STEP_IN: return s.narrow ? narrow_plan(s.g, nb, s.L).part_floats : loss::dw_plan(s.g, nb, s.L).part_floats;
        default: return 0;
    }
}

// Floats of the weight and of the bias gradient a step writes.
inline size_t step_dw_floats(const Step& s) { return s.dw >= 0 ? (size_t)s.g.Cout * s.g.Cin * s.g.k : 0; }
inline size_t step_db_floats(const Step& s) {
    if (s.db < 0) return 0;
    return s.kind == STEP_BIAS ? (size_t)s.g.Cin : (size_t)s.g.Cout;
}

struct Bufs {
    float* cot[2];
    float* gv;
    float* part;
    float* wtmp;
    float* btmp;
};
inline size_t widest_map(const Dims& d) {
    size_t n = (size_t)d.C * d.T;
    for (int k = 0; k < kStages; ++k) n = std::max(n, (size_t)stage_c(d, k) * stage_len(d, k));
    return n;
}
inline size_t part_floats(const Dims& d) {
    size_t n = 0;
    for (const Step& s : plan_steps(d)) n = std::max(n, step_part_floats(s, d.B));
    return n;
}
inline size_t widest_weight(const Dims& d) {
    size_t n = 0;
    for (const Step& s : plan_steps(d)) n = std::max(n, step_dw_floats(s));
    return n;
}
inline size_t widest_bias(const Dims& d) {
    size_t n = 0;
    for (const Step& s : plan_steps(d)) n = std::max(n, step_db_floats(s));
    return n;
}

// The one statement of the backward's workspace.
template <typename A>
void carve_backward(A& a, const Dims& d, Bufs* out) {
    Bufs b{};
    const size_t n = (size_t)d.B * widest_map(d);
    for (float*& c : b.cot) c = a.template take<float>(n);
    b.gv = a.template take<float>(n);
    b.part = a.template take<float>(part_floats(d));
    b.wtmp = a.template take<float>(widest_weight(d));
    b.btmp = a.template take<float>(widest_bias(d));
    if (out) *out = b;
}

inline std::string print_plan(const Dims& d) {
    Sizer t, w;
    carve_tape(t, d, nullptr);
    carve_backward(w, d, nullptr);
    char buf[256];
    std::snprintf(buf, sizeof(buf), "M=%d C=%d B=%d T=%d tape=%zu ws=%zu cot=%zu part=%zu", d.M, d.C, d.B, d.T,
                  t.off + 256, w.off + 256, (size_t)d.B * widest_map(d), part_floats(d));
    std::string line(buf);
    for (const Step& s : plan_steps(d)) {
        std::vector<LaunchRow> rows;
        step_rows(s, d.B, true, s.dw >= 0, s.db >= 0, rows);
        for (const LaunchRow& r : rows) {
            std::snprintf(buf, sizeof(buf), " %s:%s[grid=%ux%ux%u thr=%d lds=%zu]", s.label, r.kernel, r.gx, r.gy, r.gz,
                          r.threads, r.lds);
            line += buf;
        }
    }
    return line;
}

}  // namespace vgrad
}  // namespace m2
