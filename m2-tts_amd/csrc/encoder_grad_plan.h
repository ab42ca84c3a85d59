// The host-only half of encoder_grad.hip: the tape of TextEncoder's training forward, the workspace
// of its backward and every launch of one m2_encoder_backward call.  Pure arithmetic on the host, as
// decoder_grad_plan.h: tools/plan_check.cpp runs all of it on the CPU.
//
// The function, for ids [B, S] read as R = B S positions:
//   x_0 = emb[id] sqrt(H) + pe[s]  (an id outside [0, V) reads a zero row),
//   x_{l+1} = layer_l(x_l; key mask)  (layer_grad_plan.h),   out = LN(x_last).
// Parameters in parameters() order: embedding.weight [V, H], 11 per layer (P_* of layer_grad_plan.h),
// norm.weight and norm.bias.  The positional table is a buffer and gets no gradient.
//
// The tape: x0 [R, H], the embedding's output and layer 0's input, then the decoder's five maps per
// layer (m2_encoder_tape_map's index = 0, or 1 + 5 layer + map), each on a 256-byte boundary.
//
// The workspace is the decoder's (carve_bufs); the cotangent of x0 is written by layer 0's qx into
// cot[0], free by then, and read by the embedding's gradient.
//
// The embedding's gradient: workgroup (v, j) of emb_dw_kernel owns the vocabulary row v and the
// positions [j rps, min(R, (j + 1) rps)); it adds the rows of d_x0 whose id is v in ascending position
// and stores scale times that sum as partial j.  The split over R is this plan's own (emb_split):
// about kCUs workgroups in all, whole kEmbChunk-position chunks each, so one range per row at V >= 256.
//
// The printed form (m2_debug_encoder_grad_plan) is the decoder's, one line:
//   V= H= layers= heads= B= S= tape=<bytes> ws=<bytes> part=<floats>
// then one item per launch, <step>:<kernel>[grid=<x>x<y>x<z> thr=<threads> lds=<bytes>], <step> being
// nx (the final norm alone), the nine steps of each layer l = layers-1..0 and ew (the embedding).
#pragma once

#include "layer_grad_plan.h"

namespace m2 {
namespace egrad {

using dgrad::Bufs;
using dgrad::Geo;
using dgrad::LaunchRow;
using dgrad::Step;

constexpr int kEmbChunk = 64;   // emb_dw_kernel: positions whose ids are matched at once
constexpr int kMaxVocab = 1 << 16;
constexpr int kLrWaves = 4;     // lr_adjoint_kernel: phonemes per workgroup, one wave each

struct Dims {
    int V, H, layers, heads, B, S;
};
inline int n_params(const Dims& d) { return 1 + dgrad::kLayerParams * d.layers + 2; }
inline int n_maps(const Dims& d) { return 1 + dgrad::kLayerMaps * d.layers; }
inline int p_layer(int l, int which) { return 1 + dgrad::kLayerParams * l + which; }
inline int p_norm(const Dims& d) { return 1 + dgrad::kLayerParams * d.layers; }  // norm.weight; + 1: norm.bias
inline int map_of(int l, int which) { return 1 + dgrad::kLayerMaps * l + which; }
inline size_t rows(const Dims& d) { return (size_t)d.B * d.S; }
inline Geo geo(const Dims& d) { return {rows(d), d.B, d.S, d.H, d.heads}; }

inline bool vocab_ok(int V) { return V >= 1 && V <= kMaxVocab; }
inline bool dims_ok(const Dims& d) { return dgrad::stack_ok(d.H, d.layers, d.heads, d.B, d.S) && vocab_ok(d.V); }

inline int map_width(const Dims& d, int index) {
    return index == 0 ? d.H : dgrad::layer_map_width(d.H, (index - 1) % dgrad::kLayerMaps);
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

struct EmbPlan {
    int splits = 0, rps = 0;  // workgroups over R per vocabulary row, positions per workgroup
    size_t part_floats = 0;
};
inline bool emb_ok(int V, int H) { return vocab_ok(V) && H >= 1 && H <= 256; }
inline EmbPlan emb_split(size_t R, int V, int H) {
    EmbPlan p;
    const long long chunks = (long long)((R + kEmbChunk - 1) / kEmbChunk);
    const long long want = std::max<long long>(1, std::min<long long>(chunks, cdiv(dgrad::kCUs, V)));
    p.rps = (int)((chunks + want - 1) / want) * kEmbChunk;
    p.splits = (int)((R + p.rps - 1) / p.rps);
    p.part_floats = (size_t)p.splits * V * H;
    return p;
}
inline LaunchRow emb_row(size_t R, int V, int H) {
    return {"emb_dw_kernel", (unsigned)V, (unsigned)emb_split(R, V, H).splits, 1, 256, 0};
}

inline bool ln_ok(int K) { return K >= 8 && K % 8 == 0 && K <= dgrad::kMaxLnK; }
inline LaunchRow ln_row(size_t R, int K) {
    return {"ln_bwd_kernel", (unsigned)dgrad::dx_blocks(R), 1, 1, 256, dgrad::ln_lds_floats(K) * sizeof(float)};
}
inline size_t ln_part_floats(size_t R, int K) { return dgrad::dx_part_floats(R, K, dgrad::DX_LN); }

inline LaunchRow lr_row(int B, int S) {
    return {"lr_adjoint_kernel", (unsigned)cdiv(S, kLrWaves), (unsigned)B, 1, 64 * kLrWaves, 0};
}

// ---- the steps of one backward call ------------------------------------------------

// nx: gy = d_out, aux = the last layer's x_out, out = BUF_COT0, dgamma / dbeta = norm.weight / .bias.
// ew: gy = BUF_DX (the cotangent of x0), dw = embedding.weight, K = H, N = V.
inline std::vector<Step> plan_steps(const Dims& d) {
    std::vector<Step> s;
    const int H = d.H, L = d.layers;
    Step nx = dgrad::make_step(dgrad::STEP_LN, "nx", -1, H, H, dgrad::BUF_DMEL);
    nx.aux = egrad::map_of(L - 1, dgrad::MAP_XOUT);
    nx.out = dgrad::BUF_COT0;
    nx.dgamma = p_norm(d);
    nx.dbeta = p_norm(d) + 1;
    s.push_back(nx);
    for (int l = L - 1; l >= 0; --l)
        dgrad::layer_steps(s, H, l, p_layer(l, 0), map_of(l, 0), l == 0 ? 0 : egrad::map_of(l - 1, dgrad::MAP_XOUT),
                           l == 0 ? (int)dgrad::BUF_DX : (int)dgrad::BUF_COT0);
    Step ew = dgrad::make_step(dgrad::STEP_EMB, "ew", -1, H, d.V, dgrad::BUF_DX);
    ew.dw = 0;
    s.push_back(ew);
    return s;
}

// The launches of one step, as dgrad::step_rows (for nx, dw and db are norm.weight and norm.bias).
inline void step_rows(const Step& s, const Dims& d, bool dx, bool dw, bool db, std::vector<LaunchRow>& out) {
    switch (s.kind) {
        case dgrad::STEP_LN:
            out.push_back(ln_row(rows(d), s.K));
            if (dw) out.push_back(dgrad::finish_row((size_t)s.K));
            if (db) out.push_back(dgrad::finish_row((size_t)s.K));
            break;
        case dgrad::STEP_EMB:
            if (!dw) break;
            out.push_back(emb_row(rows(d), d.V, d.H));
            out.push_back(dgrad::finish_row((size_t)d.V * d.H));
            break;
        default: dgrad::step_rows(s, geo(d), dx, dw, db, out);
    }
}

inline size_t step_part_floats(const Step& s, const Dims& d) {
    switch (s.kind) {
        case dgrad::STEP_LN: return ln_part_floats(rows(d), s.K);
        case dgrad::STEP_EMB: return emb_split(rows(d), d.V, d.H).part_floats;
        default: return dgrad::step_part_floats(s, geo(d));
    }
}
inline size_t part_floats(const Dims& d) {
    size_t n = 0;
    for (const Step& s : plan_steps(d)) n = std::max(n, step_part_floats(s, d));
    return n;
}

// The one statement of the backward's workspace.
template <typename A>
void carve_backward(A& a, const Dims& d, Bufs* out) {
    dgrad::carve_bufs(a, geo(d), part_floats(d), out);
}

inline std::string print_plan(const Dims& d) {
    Sizer t, w;
    carve_tape(t, d, nullptr);
    carve_backward(w, d, nullptr);
    char buf[256];
    std::snprintf(buf, sizeof(buf), "V=%d H=%d layers=%d heads=%d B=%d S=%d tape=%zu ws=%zu part=%zu", d.V, d.H, d.layers,
                  d.heads, d.B, d.S, t.off + 256, w.off + 256, part_floats(d));
    std::string line(buf);
    for (const Step& s : plan_steps(d)) {
        std::vector<LaunchRow> rows_;
        const bool ln = s.kind == dgrad::STEP_LN || (s.kind == dgrad::STEP_DX && s.mode == dgrad::DX_LN);
        const bool w_ = s.kind == dgrad::STEP_DW || s.kind == dgrad::STEP_EMB;
        step_rows(s, d, true, w_ ? s.dw >= 0 : ln, w_ ? s.db >= 0 : ln, rows_);
        dgrad::print_rows(line, s.label, rows_);
    }
    return line;
}

}  // namespace egrad
}  // namespace m2
