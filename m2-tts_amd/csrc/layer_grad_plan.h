// What the gradient plans of the two transformer stacks share (decoder_grad_plan.h: MelDecoder,
// encoder_grad_plan.h: TextEncoder): the kernels' geometry, the step record, the nine steps of one
// pre-LN layer's backward, the launches of a step, the workspace's buffers and the printed row.  Pure
// arithmetic on the host, as the two plans that include it.
//
// A layer, with its input x_l:
//   qkv = LN1(x_l) Wqkv^T,  att = softmax(Q K^T / sqrt(hd), key mask) V,  x_mid = x_l + att Wo^T + bo,
//   h = relu(LN2(x_mid) W1^T + b1),  x_out = x_mid + h W2^T + b2.
// Its 11 parameters in state_dict order are P_* below and its five taped maps MAP_* (decoder_grad_plan.h
// states the tape).  Its backward walks l2w | l2x | l1w | l1x | ow | ox | att | qw | qx: the weight (w) and
// data (x) gradients of linear2, linear1, out_proj and qkv, and the attention's backward.
#pragma once

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "losses_plan.h"

namespace m2 {
namespace dgrad {

using loss::LaunchRow;

constexpr int kLayerParams = 11, kLayerMaps = 5;
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
enum Map { MAP_QKV = 0, MAP_ATT, MAP_XMID, MAP_H, MAP_XOUT };

inline bool head_dim_ok(int hd) { return hd == 16 || hd == 32 || hd == 48 || hd == 64; }
// The limits a stack of these layers puts on (H, layers, heads, B, N): N rows per utterance.
inline bool stack_ok(int H, int layers, int heads, int B, int N) {
    return H >= 8 && H % 8 == 0 && 2 * H <= kMaxK && heads >= 1 && H % heads == 0 && head_dim_ok(H / heads) &&
           layers >= 1 && layers <= kMaxLayers && B >= 0 && B <= loss::kMaxGrid && N >= 0 && N <= (1 << 22) &&
           (long long)B * N <= (1 << 24);
}
inline int layer_map_width(int H, int which) { return which == MAP_QKV ? 3 * H : which == MAP_H ? 2 * H : H; }

// The rows of one call: B utterances of N rows of H columns.
struct Geo {
    size_t R;
    int B, N, H, heads;
};

// ---- the kernels' geometry ---------------------------------------------------------

inline int col_tiles(int K) { return cdiv(K, 16); }
// Row stride of the staged B operand (16 col_tiles values of one reduction index): 16 mod 32 floats, so
// the four reduction indices a wave reads at once start 16 banks apart.
inline int b_stride(int K) { return 16 * col_tiles(K) + (col_tiles(K) % 2 == 0 ? 16 : 0); }

enum DxMode { DX_PLAIN = 0, DX_RELU = 1, DX_LN = 2 };
inline bool dx_ok(int K, int N, DxMode mode) {
    return K >= 8 && K % 8 == 0 && K <= (mode == DX_LN ? kMaxLnK : kMaxK) && N >= 1 && N <= (1 << 20);
}
// The LayerNorm backward's rows of x, (mean, rstd) per row, and the four waves' column sums.
inline size_t ln_lds_floats(int K) { return (size_t)kRows * (K + 1) + 2 * kRows + 8 * (size_t)K; }
inline size_t dx_lds_bytes(int K, DxMode mode) {
    const size_t main = (size_t)kNc * kSa + (size_t)kNc * b_stride(K);
    return std::max(main, mode == DX_LN ? ln_lds_floats(K) : 0) * sizeof(float);
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

// STEP_LN and STEP_EMB are the text encoder's own (encoder_grad_plan.h).
enum StepKind { STEP_DW = 0, STEP_DX = 1, STEP_ATT = 2, STEP_LN = 3, STEP_EMB = 4 };
// Buffers a step reads and writes: a tape map (an index >= 0) or one of these.
enum Buf { BUF_NONE = -1, BUF_X = -2, BUF_DMEL = -3, BUF_DX = -4, BUF_COT0 = -5, BUF_COT1 = -6, BUF_WIDE = -7 };
constexpr int kBufs = 8;  // a table indexed by -id holds them

struct Step {
    StepKind kind;
    char label[8];
    int layer;       // l, or -1 (outside the layers)
    int K, N;        // the linear's input and output width
    int gy;          // the cotangent of the linear's output
    int x;           // STEP_DW: the linear's input (with ln >= 0: the LayerNorm's input); STEP_ATT: qkv
    int ln;          // STEP_DW: index of the LayerNorm's weight when X is LN(x) re-formed, else -1
    int w, dw, db;   // parameter indices: the weight read (STEP_DX), the gradients written (-1: none)
    DxMode mode;     // STEP_DX
    int aux;         // STEP_DX: the taped h (DX_RELU) or the LayerNorm's input (DX_LN); STEP_ATT: att
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

// The nine steps of layer l, the cotangent of its output in BUF_COT0: p0 is the index of its first
// parameter, m0 of its first map, `in` its input and `out` where the cotangent of that input goes.
inline void layer_steps(std::vector<Step>& s, int H, int l, int p0, int m0, int in, int out) {
    const auto P = [p0](int which) { return p0 + which; };
    const auto M = [m0](int which) { return m0 + which; };
    s.push_back(dw_step("l2w", l, 2 * H, H, BUF_COT0, M(MAP_H), -1, P(P_L2_W), P(P_L2_B)));
    s.push_back(dx_step("l2x", l, 2 * H, H, BUF_COT0, P(P_L2_W), DX_RELU, M(MAP_H), BUF_NONE, BUF_WIDE, -1));
    s.push_back(dw_step("l1w", l, H, 2 * H, BUF_WIDE, M(MAP_XMID), P(P_N2_W), P(P_L1_W), P(P_L1_B)));
    s.push_back(dx_step("l1x", l, H, 2 * H, BUF_WIDE, P(P_L1_W), DX_LN, M(MAP_XMID), BUF_COT0, BUF_COT1, P(P_N2_W)));
    s.push_back(dw_step("ow", l, H, H, BUF_COT1, M(MAP_ATT), -1, P(P_OUT_W), P(P_OUT_B)));
    s.push_back(dx_step("ox", l, H, H, BUF_COT1, P(P_OUT_W), DX_PLAIN, BUF_NONE, BUF_NONE, BUF_COT0, -1));
    Step att = make_step(STEP_ATT, "att", l, H, 3 * H, BUF_COT0);
    att.x = M(MAP_QKV);
    att.aux = M(MAP_ATT);
    s.push_back(att);
    s.push_back(dw_step("qw", l, H, 3 * H, BUF_WIDE, in, P(P_N1_W), P(P_QKV_W), -1));
    s.push_back(dx_step("qx", l, H, 3 * H, BUF_WIDE, P(P_QKV_W), DX_LN, in, BUF_COT1, out, P(P_N1_W)));
}

// The launches of one step of the layer walk; dx: its data gradient is asked for, dw, db: which of its
// parameter gradients (for DX_LN: the LayerNorm's weight and bias).
inline void step_rows(const Step& s, const Geo& g, bool dx, bool dw, bool db, std::vector<LaunchRow>& out) {
    switch (s.kind) {
        case STEP_DW: {
            if (!dw && !db) break;
            const DwPlan p = dw_split(g.R, s.K, s.N);
            out.push_back({"lin_dw_kernel", (unsigned)p.tiles, (unsigned)p.splits, 1, 256, p.lds});
            if (dw) out.push_back(finish_row((size_t)s.N * s.K));
            if (db) out.push_back(finish_row((size_t)s.N));
            break;
        }
        case STEP_DX:
            if (!dx && !dw && !db) break;
            out.push_back(dx_row(g.R, s.K, s.mode));
            if (dw) out.push_back(finish_row((size_t)s.K));
            if (db) out.push_back(finish_row((size_t)s.K));
            break;
        case STEP_ATT: {
            const unsigned gx = (unsigned)cdiv(g.N, kRows);
            const size_t lds = att_lds_bytes(g.H / g.heads);
            out.push_back({"att_bwd_q_kernel", gx, (unsigned)g.heads, (unsigned)g.B, 256, lds});
            out.push_back({"att_bwd_kv_kernel", gx, (unsigned)g.heads, (unsigned)g.B, 256, lds});
            break;
        }
        default: break;
    }
}

// Floats of partials a step needs in the workspace.
inline size_t step_part_floats(const Step& s, const Geo& g) {
    switch (s.kind) {
        case STEP_DW: return dw_split(g.R, s.K, s.N).part_floats;
        case STEP_DX: return dx_part_floats(g.R, s.K, s.mode);
        default: return 0;
    }
}

struct Bufs {
    float* cot[2];
    float* wide;
    float* stats;
    float* part;
};

// The one statement of a backward's workspace: two cotangent maps [R, H], one [R, 3H], the attention's
// row statistics and `part` floats of partials.
template <typename A>
void carve_bufs(A& a, const Geo& g, size_t part, Bufs* out) {
    Bufs b{};
    for (float*& c : b.cot) c = a.template take<float>(g.R * g.H);
    b.wide = a.template take<float>(g.R * 3 * g.H);
    b.stats = a.template take<float>(att_stat_floats(g.B, g.heads, g.N));
    b.part = a.template take<float>(part);
    if (out) *out = b;
}

// " <step>:<kernel>[grid=<x>x<y>x<z> thr=<threads> lds=<bytes>]" per row.
inline void print_rows(std::string& line, const char* label, const std::vector<LaunchRow>& rows) {
    char buf[256];
    for (const LaunchRow& r : rows) {
        std::snprintf(buf, sizeof(buf), " %s:%s[grid=%ux%ux%u thr=%d lds=%zu]", label, r.kernel, r.gx, r.gy, r.gz,
                      r.threads, r.lds);
        line += buf;
    }
}

}  // namespace dgrad
}  // namespace m2
