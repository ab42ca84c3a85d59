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

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "losses_plan.h"

namespace m2 {
namespace dgrad {

using loss::LaunchRow;

constexpr int kLayerParams = 11, kTailParams = 4, kLayerMaps = 5;
constexpr int kMaxLayers = 64;
constexpr int kRows = 64;   // rows of a lin_dx workgroup; queries / keys of an attention workgroup
constexpr int kNc = 32;     // lin_dx_kernel: rows of W per LDS chunk of the reduction over N
constexpr int kRc = 32;     // lin_dw_kernel: rows of g_y and X per LDS chunk of the reduction over R
constexpr int kSa = 65;     // row stride of the staged A operand (64 values of one reduction index)
constexpr int kCUs = 256;   // compute units of the part the split is sized for
constexpr int kFinE = 32;   // dec_finish_kernel: elements per workgroup,
constexpr int kFinG = 8;    // each summed by this many threads over interleaved slots
constexpr int kMaxK = 256;  // widest output row of lin_dx / lin_dw (2H)
constexpr int kMaxLnK = 128;  // widest row the LayerNorm-backward epilogue holds (H)

enum LayerParam { P_QKV_W = 0, P_OUT_W, P_OUT_B, P_L1_W, P_L1_B, P_L2_W, P_L2_B, P_N1_W, P_N1_B, P_N2_W, P_N2_B };
enum TailParam { T_N_W = 0, T_N_B, T_MEL_W, T_MEL_B };
enum Map { MAP_QKV = 0, MAP_ATT, MAP_XMID, MAP_H, MAP_XOUT };

struct Dims {
    int H, M, layers, heads, B, T;
};
inline int n_params(const Dims& d) { return kLayerParams * d.layers + kTailParams; }
inline int n_maps(const Dims& d) { return kLayerMaps * d.layers; }
inline int p_layer(int l, int which) { return kLayerParams * l + which; }
inline int p_tail(const Dims& d, int which) { return kLayerParams * d.layers + which; }
inline size_t rows(const Dims& d) { return (size_t)d.B * d.T; }

inline bool head_dim_ok(int hd) { return hd == 16 || hd == 32 || hd == 48 || hd == 64; }
inline bool dims_ok(const Dims& d) {
    return d.H >= 8 && d.H % 8 == 0 && 2 * d.H <= kMaxK && d.heads >= 1 && d.H % d.heads == 0 &&
           head_dim_ok(d.H / d.heads) && d.M >= 1 && d.M <= (1 << 16) && d.layers >= 1 && d.layers <= kMaxLayers &&
           d.B >= 0 && d.B <= loss::kMaxGrid && d.T >= 0 && d.T <= (1 << 22) && (long long)d.B * d.T <= (1 << 24);
}

inline int map_width(const Dims& d, int index) {
    switch (index % kLayerMaps) {
        case MAP_QKV: return 3 * d.H;
        case MAP_H: return 2 * d.H;
        default: return d.H;
    }
}

// The one statement of the tape: over a Sizer the byte count, over a Carve the maps.
template <typename A>
void carve_tape(A& a, const Dims& d, float** maps) {
    for (int i = 0; i < n_maps(d); ++i) {
        float* p = a.template take<float>(rows(d) * map_width(d, i));
        if (maps) maps[i] = p;
    }
}

// ---- the kernels' geometry ---------------------------------------------------------

inline int col_tiles(int K) { return cdiv(K, 16); }
// Row stride of the staged B operand (16 col_tiles values of one reduction index): 16 mod 32 floats, so
// the four reduction indices a wave reads at once start 16 banks apart.
inline int b_stride(int K) { return 16 * col_tiles(K) + (col_tiles(K) % 2 == 0 ? 16 : 0); }

enum DxMode { DX_PLAIN = 0, DX_RELU = 1, DX_LN = 2 };
inline bool dx_ok(int K, int N, DxMode mode) {
    return K >= 8 && K % 8 == 0 && K <= (mode == DX_LN ? kMaxLnK : kMaxK) && N >= 1 && N <= (1 << 20);
}
inline size_t dx_lds_bytes(int K, DxMode mode) {
    const size_t main = (size_t)kNc * kSa + (size_t)kNc * b_stride(K);
    // the epilogue's rows of x, (mean, rstd) per row, and the four waves' column sums
    const size_t ln = mode == DX_LN ? (size_t)kRows * (K + 1) + 2 * kRows + 8 * (size_t)K : 0;
    return std::max(main, ln) * sizeof(float);
}
inline int dx_blocks(size_t R) { return (int)((R + kRows - 1) / kRows); }
inline size_t dx_part_floats(size_t R, int K, DxMode mode) { return mode == DX_LN ? (size_t)dx_blocks(R) * 2 * K : 0; }
inline LaunchRow dx_row(size_t R, int K, DxMode mode) {
    return {"lin_dx_kernel", (unsigned)dx_blocks(R), 1, 1, 256, dx_lds_bytes(K, mode)};
}

struct DwPlan {
    int tiles = 0, splits = 0, rps = 0;  // 64-row tiles of N, workgroups over R, rows per workgroup
    size_t lds = 0, part_floats = 0;
};
inline bool dw_ok(int K, int N) { return K >= 8 && K % 8 == 0 && K <= kMaxK && N >= 1 && N <= (1 << 20); }
inline DwPlan dw_split(size_t R, int K, int N) {
    DwPlan p;
    p.tiles = cdiv(N, kRows);
    const long long chunks = (long long)((R + kRc - 1) / kRc);
    const long long want = std::max<long long>(1, std::min<long long>(chunks, cdiv(kCUs, p.tiles)));
    p.rps = (int)((chunks + want - 1) / want) * kRc;
    p.splits = (int)((R + p.rps - 1) / p.rps);
    p.lds = ((size_t)kRc * kSa + (size_t)kRc * b_stride(K)) * sizeof(float);
    p.part_floats = (size_t)p.splits * ((size_t)N * K + N);
    return p;
}
inline LaunchRow finish_row(size_t n) { return {"dec_finish_kernel", (unsigned)((n + kFinE - 1) / kFinE), 1, 1, 256, 0}; }

inline size_t att_lds_bytes(int hd) { return ((size_t)2 * hd * (kRows + 4) + 3 * kRows) * sizeof(float); }
inline size_t att_stat_floats(int B, int heads, int N) { return (size_t)B * heads * N * 3; }

// ---- the steps of one backward call ------------------------------------------------

enum StepKind { STEP_DW = 0, STEP_DX = 1, STEP_ATT = 2 };
// Buffers a step reads and writes: a tape map (0 .. 5 layers - 1) or one of these.
enum Buf { BUF_NONE = -1, BUF_X = -2, BUF_DMEL = -3, BUF_DX = -4, BUF_COT0 = -5, BUF_COT1 = -6, BUF_WIDE = -7 };

struct Step {
    StepKind kind;
    char label[8];
    int layer;       // l, or -1 (the final norm and mel_projection)
    int K, N;        // the linear's input and output width
    int gy;          // the cotangent of the linear's output
    int x;           // STEP_DW: the linear's input (with ln >= 0: the LayerNorm's input)
    int ln;          // STEP_DW: index of the LayerNorm's weight when X is LN(x) re-formed, else -1
    int w, dw, db;   // parameter indices: the weight read (STEP_DX), the gradients written (-1: none)
    DxMode mode;     // STEP_DX
    int aux;         // STEP_DX: the taped h (DX_RELU) or the LayerNorm's input (DX_LN)
    int res;         // DX_LN: the residual branch's cotangent, or BUF_NONE
    int out;         // STEP_DX: g_x
    int dgamma, dbeta;  // DX_LN: the LayerNorm's gradients (gamma = dgamma's parameter)
};

inline Step make_step(StepKind kind, const char* name, int l, int K, int N, int gy) {
    Step s{};
    s.kind = kind;
    s.layer = l;
    if (l >= 0) std::snprintf(s.label, sizeof(s.label), "%s%d", name, l);
    else std::snprintf(s.label, sizeof(s.label), "%s", name);
    s.K = K;
    s.N = N;
    s.gy = gy;
    s.x = s.aux = s.res = s.out = BUF_NONE;
    s.ln = s.w = s.dw = s.db = s.dgamma = s.dbeta = -1;
    s.mode = DX_PLAIN;
    return s;
}
inline Step dw_step(const char* name, int l, int K, int N, int gy, int x, int ln, int dw, int db) {
    Step s = make_step(STEP_DW, name, l, K, N, gy);
    s.x = x;
    s.ln = ln;
    s.dw = dw;
    s.db = db;
    return s;
}
inline Step dx_step(const char* name, int l, int K, int N, int gy, int w, DxMode mode, int aux, int res, int out,
                    int gamma) {
    Step s = make_step(STEP_DX, name, l, K, N, gy);
    s.w = w;
    s.mode = mode;
    s.aux = aux;
    s.res = res;
    s.out = out;
    if (mode == DX_LN) {
        s.dgamma = gamma;
        s.dbeta = gamma + 1;
    }
    return s;
}

inline int map_of(int l, int which) { return kLayerMaps * l + which; }
// The input of layer l: the caller's x, or the layer below's x_out.
inline int layer_input(int l) { return l == 0 ? (int)BUF_X : map_of(l - 1, MAP_XOUT); }

inline std::vector<Step> plan_steps(const Dims& d) {
    std::vector<Step> s;
    const int H = d.H, L = d.layers;
    const int last = map_of(L - 1, MAP_XOUT);
    s.push_back(dw_step("mw", -1, H, d.M, BUF_DMEL, last, p_tail(d, T_N_W), p_tail(d, T_MEL_W), p_tail(d, T_MEL_B)));
    s.push_back(dx_step("mx", -1, H, d.M, BUF_DMEL, p_tail(d, T_MEL_W), DX_LN, last, BUF_NONE, BUF_COT0,
                        p_tail(d, T_N_W)));
    for (int l = L - 1; l >= 0; --l) {
        const int in = layer_input(l);
        s.push_back(dw_step("l2w", l, 2 * H, H, BUF_COT0, map_of(l, MAP_H), -1, p_layer(l, P_L2_W), p_layer(l, P_L2_B)));
        s.push_back(dx_step("l2x", l, 2 * H, H, BUF_COT0, p_layer(l, P_L2_W), DX_RELU, map_of(l, MAP_H), BUF_NONE,
                            BUF_WIDE, -1));
        s.push_back(dw_step("l1w", l, H, 2 * H, BUF_WIDE, map_of(l, MAP_XMID), p_layer(l, P_N2_W), p_layer(l, P_L1_W),
                            p_layer(l, P_L1_B)));
        s.push_back(dx_step("l1x", l, H, 2 * H, BUF_WIDE, p_layer(l, P_L1_W), DX_LN, map_of(l, MAP_XMID), BUF_COT0,
                            BUF_COT1, p_layer(l, P_N2_W)));
        s.push_back(dw_step("ow", l, H, H, BUF_COT1, map_of(l, MAP_ATT), -1, p_layer(l, P_OUT_W), p_layer(l, P_OUT_B)));
        s.push_back(dx_step("ox", l, H, H, BUF_COT1, p_layer(l, P_OUT_W), DX_PLAIN, BUF_NONE, BUF_NONE, BUF_COT0, -1));
        s.push_back(make_step(STEP_ATT, "att", l, H, 3 * H, BUF_COT0));
        s.push_back(dw_step("qw", l, H, 3 * H, BUF_WIDE, in, p_layer(l, P_N1_W), p_layer(l, P_QKV_W), -1));
        s.push_back(dx_step("qx", l, H, 3 * H, BUF_WIDE, p_layer(l, P_QKV_W), DX_LN, in, BUF_COT1,
                            l == 0 ? (int)BUF_DX : (int)BUF_COT0, p_layer(l, P_N1_W)));
    }
    return s;
}

// The launches of one step; dx: its data gradient is asked for (always, but for layer 0's input),
// dw, db: which of its parameter gradients (for DX_LN: the LayerNorm's weight and bias).
inline void step_rows(const Step& s, const Dims& d, bool dx, bool dw, bool db, std::vector<LaunchRow>& out) {
    const size_t R = rows(d);
    switch (s.kind) {
        case STEP_DW: {
            if (!dw && !db) break;
            const DwPlan p = dw_split(R, s.K, s.N);
            out.push_back({"lin_dw_kernel", (unsigned)p.tiles, (unsigned)p.splits, 1, 256, p.lds});
            if (dw) out.push_back(finish_row((size_t)s.N * s.K));
            if (db) out.push_back(finish_row((size_t)s.N));
            break;
        }
        case STEP_DX:
            if (!dx && !dw && !db) break;
            out.push_back(dx_row(R, s.K, s.mode));
            if (dw) out.push_back(finish_row((size_t)s.K));
            if (db) out.push_back(finish_row((size_t)s.K));
            break;
        case STEP_ATT: {
            const unsigned gx = (unsigned)cdiv(d.T, kRows);
            const size_t lds = att_lds_bytes(d.H / d.heads);
            out.push_back({"att_bwd_q_kernel", gx, (unsigned)d.heads, (unsigned)d.B, 256, lds});
            out.push_back({"att_bwd_kv_kernel", gx, (unsigned)d.heads, (unsigned)d.B, 256, lds});
            break;
        }
    }
}

// Floats of partials a step needs in the workspace.
inline size_t step_part_floats(const Step& s, const Dims& d) {
    switch (s.kind) {
        case STEP_DW: return dw_split(rows(d), s.K, s.N).part_floats;
        case STEP_DX: return dx_part_floats(rows(d), s.K, s.mode);
        default: return 0;
    }
}
inline size_t part_floats(const Dims& d) {
    size_t n = 0;
    for (const Step& s : plan_steps(d)) n = std::max(n, step_part_floats(s, d));
    return n;
}

struct Bufs {
    float* cot[2];
    float* wide;
    float* stats;
    float* part;
};

// The one statement of the backward's workspace.
template <typename A>
void carve_backward(A& a, const Dims& d, Bufs* out) {
    Bufs b{};
    const size_t R = rows(d);
    for (float*& c : b.cot) c = a.template take<float>(R * d.H);
    b.wide = a.template take<float>(R * 3 * d.H);
    b.stats = a.template take<float>(att_stat_floats(d.B, d.heads, d.T));
    b.part = a.template take<float>(part_floats(d));
    if (out) *out = b;
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
        for (const LaunchRow& r : rows_) {
            std::snprintf(buf, sizeof(buf), " %s:%s[grid=%ux%ux%u thr=%d lds=%zu]", s.label, r.kernel, r.gx, r.gy, r.gz,
                          r.threads, r.lds);
            line += buf;
        }
    }
    return line;
}

}  // namespace dgrad
}  // namespace m2
