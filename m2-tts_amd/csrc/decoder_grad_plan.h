// The host-only half of decoder_grad.hip: the tape of MelDecoder's training forward, the workspace
// of its backward and every launch of one m2_decoder_backward call.  Pure arithmetic on the host:
// nothing here touches a device, so tools/plan_check.cpp runs all of it on the CPU.  Both _bytes
// queries run the carves over a Sizer and both calls run them over a Carve before anything is
// launched; m2_decoder_backward walks plan_steps() and launches what each step's rows name.
//
// The function, for x [B, T, H] read as R = B T rows.  Per layer, with the layer's input x_l:
//   qkv = LN1(x_l) Wqkv^T,  att = softmax(Q K^T / sqrt(hd)) V,  x_mid = x_l + att Wo^T + bo,
//   h = relu(LN2(x_mid) W1^T + b1),  x_out = x_mid + h W2^T + b2;   mel = LN(x_last) Wm^T + bm.
// Parameters in state_dict order, 11 per layer (P_* below) and 4 behind them (T_*).
//
// The tape, stated once.  Maps are float32 [R, width], each on a 256-byte boundary, five per layer
// in this order (m2_decoder_tape_map's index = 5 layer + map):
//    0  qkv    [R, 3H]
//    1  att    [R, H]
//    2  x_mid  [R, H]
//    3  h      [R, 2H]   post-ReLU: relu' reads the forward's own predicate, h > 0
//    4  x_out  [R, H]    the next layer's input, the final norm's after the last layer
// Layer 0's input is the caller's x.  LayerNorm statistics and attention probabilities are not
// taped: the backward recomputes them.
//
// The workspace: two cotangent maps [R, H] (cot[0]: of a layer's output, then of att and of the
// layer's input; cot[1]: of x_mid), one [R, 3H] (g_h, then d_qkv), the attention's row statistics
// [B, heads, T, 3] (max, 1 / sum, D) and the partials of the widest reduction (`part`).  With
// `accumulate` a gradient's partials are summed exactly as without it and the finish adds that sum
// onto the caller's tensor: one fp32 addition per element.
//
// The weight gradient's split over R is this plan's own (dw_split): enough workgroups to cover
// kCUs compute units at R = 16000 whatever the layer's width, at least one kRc-row chunk each.
//
// The printed form (m2_debug_decoder_grad_plan) is one line of space-separated items, fixed:
//   H= M= layers= heads= B= T= tape=<bytes> ws=<bytes> part=<floats>
// then one item per launch, in launch order,
//   <step>:<kernel>[grid=<x>x<y>x<z> thr=<threads> lds=<bytes>]
// <step> is mw | mx, then per layer l = layers-1..0: l2w<l> | l2x<l> | l1w<l> | l1x<l> | ow<l> |
// ox<l> | att<l> | qw<l> | qx<l>: the weight (w) and data (x) gradients of mel_projection, linear2,
// linear1, out_proj and qkv, and the attention's backward.  The line is that of a call with every
// gradient and d_x asked for.
#pragma once

#include "layer_grad_plan.h"

namespace m2 {
namespace dgrad {

constexpr int kTailParams = 4;
enum TailParam { T_N_W = 0, T_N_B, T_MEL_W, T_MEL_B };

struct Dims {
    int H, M, layers, heads, B, T;
};
inline int n_params(const Dims& d) { return kLayerParams * d.layers + kTailParams; }
inline int n_maps(const Dims& d) { return kLayerMaps * d.layers; }
inline int p_layer(int l, int which) { return kLayerParams * l + which; }
inline int p_tail(const Dims& d, int which) { return kLayerParams * d.layers + which; }
inline size_t rows(const Dims& d) { return (size_t)d.B * d.T; }
inline Geo geo(const Dims& d) { return {rows(d), d.B, d.T, d.H, d.heads}; }

inline bool dims_ok(const Dims& d) {
    return stack_ok(d.H, d.layers, d.heads, d.B, d.T) && d.M >= 1 && d.M <= (1 << 16);
}

inline int map_width(const Dims& d, int index) { return layer_map_width(d.H, index % kLayerMaps); }

// The one statement of the tape: over a Sizer the byte count, over a Carve the maps.
template <typename A>
void carve_tape(A& a, const Dims& d, float** maps) {
    for (int i = 0; i < n_maps(d); ++i) {
        float* p = a.template take<float>(rows(d) * map_width(d, i));
        if (maps) maps[i] = p;
    }
}

inline int map_of(int l, int which) { return kLayerMaps * l + which; }
// The input of layer l: the caller's x, or the layer below's x_out.
inline int layer_input(int l) { return l == 0 ? (int)BUF_X : map_of(l - 1, MAP_XOUT); }

// mw | mx, then the layers' steps (layer_grad_plan.h) from the last layer down; layer 0's qx writes d_x.
inline std::vector<Step> plan_steps(const Dims& d) {
    std::vector<Step> s;
    const int H = d.H, L = d.layers;
    const int last = map_of(L - 1, MAP_XOUT);
    s.push_back(dw_step("mw", -1, H, d.M, BUF_DMEL, last, p_tail(d, T_N_W), p_tail(d, T_MEL_W), p_tail(d, T_MEL_B)));
    s.push_back(dx_step("mx", -1, H, d.M, BUF_DMEL, p_tail(d, T_MEL_W), DX_LN, last, BUF_NONE, BUF_COT0,
                        p_tail(d, T_N_W)));
    for (int l = L - 1; l >= 0; --l)
        layer_steps(s, H, l, p_layer(l, 0), map_of(l, 0), layer_input(l), l == 0 ? (int)BUF_DX : (int)BUF_COT0);
    return s;
}

inline void step_rows(const Step& s, const Dims& d, bool dx, bool dw, bool db, std::vector<LaunchRow>& out) {
    step_rows(s, geo(d), dx, dw, db, out);
}
inline size_t step_part_floats(const Step& s, const Dims& d) { return step_part_floats(s, geo(d)); }
inline size_t part_floats(const Dims& d) {
    size_t n = 0;
    for (const Step& s : plan_steps(d)) n = std::max(n, step_part_floats(s, d));
    return n;
}

// The one statement of the backward's workspace.
template <typename A>
void carve_backward(A& a, const Dims& d, Bufs* out) {
    carve_bufs(a, geo(d), part_floats(d), out);
}

inline std::string print_plan(const Dims& d) {
    Sizer t, w;
    carve_tape(t, d, nullptr);
    carve_backward(w, d, nullptr);
    char buf[256];
    std::snprintf(buf, sizeof(buf), "H=%d M=%d layers=%d heads=%d B=%d T=%d tape=%zu ws=%zu part=%zu", d.H, d.M, d.layers,
                  d.heads, d.B, d.T, t.off + 256, w.off + 256, part_floats(d));
    std::string line(buf);
    for (const Step& s : plan_steps(d)) {
        std::vector<LaunchRow> rows_;
        const bool ln = s.kind == STEP_DX && s.mode == DX_LN;
        step_rows(s, d, true, s.kind == STEP_DW ? s.dw >= 0 : ln, s.kind == STEP_DW ? s.db >= 0 : ln, rows_);
        print_rows(line, s.label, rows_);
    }
    return line;
}

}  // namespace dgrad
}  // namespace m2
