// The transformer stacks' launch plan: which kernels one text-encoder or
// mel-decoder forward launches, in which order and with what tile geometry.
// Host arithmetic only - no HIP call and no sw(): the switch table is an
// argument, so tools/plan_check.cpp runs every rule on the CPU.
// text_encoder_layers and mel_decoder (m2_runtime.hip) plan once per call and
// run_tf_plan launches what each row names; the launchers
// (transformer_layer.hip, transformer_fused.hip) take rb / qs2 / waves from
// the row.  The shape predicates of those kernels live here too, because the
// plan and the handle's creation ask them.
//
// A call runs in one of four forms (TfPlan::form, m2_debug_transformer_form):
//   3  one launch per layer (transformer_layer.hip): tfl_first, then a
//      tfl_layer per layer; the last one runs the final LN -> projection when
//      its width has an instance (next=2, `projected`)
//   2  three launches per layer, the next layer's LN1 -> QKV (or the final
//      LN -> projection) chained into post_attn_next
//   1  the same with every LN1 -> QKV its own ln_gemm launch (M2_TF_CHAIN=0)
//   0  five fp32 linears per layer around the attention
// The first launch takes its rows as given (src=x), from the embedding
// (embed) or from the length regulator's frame expansion (expand); where no
// launch builds them on the way, embed_pe / lr_expand runs first.  A decoder
// call that no layer projected ends with final_ln_gemm (packed weights, where
// (H, width) has an instance) or final_linear (fp32 weights).
//
// Outside the plan: the geometry inside launch_attention, launch_linear,
// launch_embed_pe and launch_lr_expand (also the per-op entry points;
// M2_ATT_QT / M2_ATT_F32 are theirs) - their rows carry the kind only - and
// the encoder's final LayerNorm, which m2_text_encoder launches and the
// inference front folds into the duration kernel.  A width without a kernel
// instance stays the launcher's M2_E_SHAPE.
//
// The printed form of a plan (TfPlan::print, m2_debug_transformer_plan) is
// one line of space-separated items, fixed:
//   enc|dec form=<0-3> H= heads= layers= B= N= src=x|embed|expand masked=0|1
//   devT=0|1 ragged=0|1 projected=0|1
// then one item per launch, in launch order, <kind><layer>[fields] with
//   embed_pe  lr_expand  attention<l>                     (no fields)
//   linear<l>[op=0..3]                 (LN1->QKV, out, LN2->FF1, FF2)
//   ln_gemm<l> embed_ln_gemm<l> expand_ln_gemm<l> post_attn<l> final_ln_gemm
//                                      [waves= grid= thr=]
//   post_attn_next<l>                  [next=1|2 waves= grid= thr=]
//   tfl_first<l>                       [rb= grid= thr=]
//   tfl_layer<l>                       [next=0|1|2 rb= qs2= grid= thr=]
//   final_linear                       (no fields)
// or, when the call cannot run, error="<text>" in place of the launches.
// Every field of the plan is on the line.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include "m2_common.h"

namespace m2 {

// ---------------------------------------------------------------------------
// Shape predicates.

// The one-launch layers cover (H, heads): heads == 2, H in {32, 64, 96}.
constexpr bool tfl_supported(int H, int heads) { return heads == 2 && (H == 32 || H == 64 || H == 96); }
// Final-projection widths the last one-launch decoder layer can fuse (mel channels).
constexpr bool tfl_proj_supported(int H, int NN) {
    return (H == 32 && (NN == 32 || NN == 64)) || (H == 64 && (NN == 64 || NN == 80)) ||
           (H == 96 && (NN == 80 || NN == 96));
}
// a multiple of 64 so that 16-, 32- and 64-row tiles all cover [0, npad) exactly
constexpr int tfl_npad(int N) { return (N + 63) / 64 * 64; }
// Hidden sizes with fused-layer instantiations (N_out: output width of ln_gemm).
constexpr bool tf_fused_supported(int H, int N_out) { return (H == 32 || H == 64 || H == 96) && N_out % 16 == 0; }
// post_attn followed by LN -> GEMM with NN output columns: the instances.
constexpr bool tf_post_next_supported(int H, int NN) {
    return (H == 32 && (NN == 96 || NN == 32 || NN == 64)) || (H == 64 && (NN == 192 || NN == 64 || NN == 80)) ||
           (H == 96 && (NN == 288 || NN == 80 || NN == 96));
}
// The widths launch_ln_gemm instantiates are those post_attn_kernel chains.
constexpr bool tf_ln_gemm_supported(int K, int N) { return tf_post_next_supported(K, N); }
// LN1 -> QKV with its input rows built in the same launch (embedding / frame expansion).
constexpr bool tf_src_fused_supported(int H, int N) {
    return (H == 32 && N == 96) || (H == 64 && N == 192) || (H == 96 && N == 288);
}

// ---------------------------------------------------------------------------
// Tile rules of the one-launch layers (transformer_layer.hip asserts its own
// constants against these).
namespace tfl {
constexpr int kTileRows = 16;  // rows (queries) of one tile; a workgroup owns rb of them
constexpr int kWaves = 8;      // waves per layer workgroup
// Waves per first-launch workgroup: 64-row tiles (the very large grids) run
// 4 waves, so two workgroups share a CU at 189 VGPRs and one tile's latency
// chain (prefix sums -> search -> gather -> LN -> QKV -> stores) overlaps the
// other's: configs[4]'s frame-expansion launch 210 -> 192 us; the small grids'
// 16- and 32-row tiles keep 8 (4 there: B=8 6.3 -> 7.5 us,
// profiles/r04/r04af_*).
#ifndef FK_NW4  // A/B builds: waves of the 64-row-tile workgroups
#define FK_NW4 4
#endif
constexpr int fk_nw(int rb) { return rb == 4 ? FK_NW4 : kWaves; }
}  // namespace tfl

inline long tfl_tiles16(int B, int N) { return (long)B * (tfl_npad(N) / tfl::kTileRows); }

// Rows per workgroup of the layer launches: 64 (query-split attention, K / V
// staged in LDS) once the 64-row tiles alone fill the 256 CUs; else 16 while
// one round of the CUs holds the 16-row grid, else 32.  M2_TFL_RB=1|2|4
// forces one.  The first (LN1 -> QKV) launch has no attention: at most 32.
inline int tfl_rb(int B, int N, const Switches& s) {
    if (s.tfl_rb) return s.tfl_rb;
    const long tiles16 = tfl_tiles16(B, N);
    return tiles16 >= 4 * 256 ? 4 : (tiles16 > 256 ? 2 : 1);
}
// The layer launches: M2_TFL_RB_MASKED / M2_TFL_RB_UNMASKED override tfl_rb.
inline int tfl_layer_rb(int B, int N, bool masked, const Switches& s) {
    return masked && s.tfl_rb_masked ? s.tfl_rb_masked : !masked && s.tfl_rb_unmasked ? s.tfl_rb_unmasked : tfl_rb(B, N, s);
}
// The first launch's rows per workgroup: the layers' choice up to 32, 64 for
// grids of >= 8 rounds of 16-row tiles (latency-bound rounds; with 8-wave
// workgroups 64-row tiles made stage2 B=64 1.4 % slower,
// profiles/r03/ab/r03x_ab.txt, with the 4-wave ones (fk_nw) 0.5-1.7 % faster,
// r04ag_s2_b64_first_rb); M2_TFL_FIRST_RB=1|2|4 forces one, then the
// masked / unmasked overrides.
inline int tfl_first_rb(int B, int N, bool masked, const Switches& s) {
    int rb = tfl_rb(B, N, s) > 1 ? 2 : 1;
    if (tfl_tiles16(B, N) >= 8L * 256) rb = 4;
    if (s.tfl_first_rb) rb = s.tfl_first_rb;
    if (masked && s.tfl_rb_masked) rb = s.tfl_rb_masked;
    if (!masked && s.tfl_rb_unmasked) rb = s.tfl_rb_unmasked;
    return rb;
}
// 64-row tiles: two query blocks per wave with the lean softmax
// (attention_qsplit2<..., LEAN>) at head_dim 48 (stage2: B=128 T=2600 step
// -1.5 %, B=16 T=2600 -1.9 %, B=64 T=500 -0.8 % against the plain two-block
// form, which was itself -0.7 % at B=128 T=2600 against one block; the lean
// one-block form +2.2 % at B=16 T=2600), the lean one-block form below
// (stage1 B=32: -0.7 % against the plain one-block form; two blocks +0.3 to
// +0.6 %; in-process A/Bs, profiles/r03/r03ab_*, r03ad_ab.txt, r03aj_ab.txt,
// r03al_ab.txt).  Round 4: at head_dim 48 the wave-specialised form with
// LDS-DMA staging (attention_qsplit_ws<..., DMA>; masked launches keep the
// lean two-block form): against the ping-pong form (6), itself -0.9 % on the
// long-form step against the lean two-block form (3): long-form step -1.5 %,
// B=16 T=2600 -1.1 %, B=64 T=500 level (in-process A/Bs,
// profiles/r04/r04j_*, r04l_*, r04m_*, r04n_*); at head_dim 32 it is slower
// than the lean one-block form (stage1 B=32 +0.5 %, B=128 +1.4 %).  Measured
// and not kept (removed in round 5): the software-pipelined form (5, level or
// slower, r04d / r04e), the wave-specialised form with register staging (7,
// between 6 and 9) and with its regions interleaved by group barriers (8,
// +3 %; 10).  Round 6: the key-quarter form (12, attention_quarters) for
// every unmasked layer - at head_dim 48 it replaces 9 (configs[4] step -4.2 %,
// B=16 T=2600 -7.1 %, B=64 T=500 -2.6 %; 9 removed, history keeps it), at
// head_dim 32 the lean one-block form (stage1 B=128 S=130 -3.2 %, B=32 S=520
// -9.1 %; profiles/r06/r06ad_*, r06ah_*).  M2_TFL_QS2=0|2|3|4|12 forces a
// form (switch table, m2_common.h): 0 / 2 one / two query blocks, 3 / 4 the
// same with the lean softmax, 12 the key-quarter form (unmasked layers).
// Form 12 is unmasked-only, and at head_dim 48 keeps the softmax base as an
// f16 pair: a masked launch, or a layer whose scores may leave the f16 range
// (wide_scores), runs the previous default instead - the lean two-block form
// 3 at head_dim 48, the one-block form 4 below.
inline int tfl_qs2(int H, int heads, bool masked, bool wide_scores, const Switches& s) {
    const int qs2 = s.tfl_qs2 >= 0 ? s.tfl_qs2 : 12;
    if (qs2 == 12 && (masked || wide_scores)) return H / heads >= 48 ? 3 : 4;
    return qs2;
}
inline int tfl_ntile(int N, int rb) { return (tfl_npad(N) + tfl::kTileRows * rb - 1) / (tfl::kTileRows * rb); }
inline int tfl_grid(int B, int N, int rb) { return B * tfl_ntile(N, rb); }

// Tile rule of the three-launch layers' GEMM kernels (transformer_fused.hip):
// a workgroup owns 32 rows.  Waves per workgroup: 8 when the grid is short of
// two workgroups per CU (small batches: every 32-row tile is then a serial
// chain of GEMM rounds, and 8 waves halve the rounds: post_attn at stage2 B=8
// S=100 13.8 -> 10.5 us, tools/probe/tf_waves_ab.sh), else 4.  M2_TF_WAVES=4|8
// forces one.  (An L2 warm-up of the layer's weights at kernel start measured
// 1 us slower: across steps they stay L2-resident.)
constexpr int kTfTileRows = 32;
inline int tf_grid(int R) { return cdiv(R, kTfTileRows); }
inline int tf_waves(int R, const Switches& s) {
    if (s.tf_waves) return s.tf_waves;
    return tf_grid(R) < 2 * 256 ? 8 : 4;
}

// ---------------------------------------------------------------------------
// The call and its plan.
enum class TfSrc : uint8_t { X = 0, Embed = 1, Expand = 2 };  // the numbering of TflFirst::src

struct TfCall {
    bool decoder = false;  // the stack: text encoder / mel decoder
    int H = 0, heads = 0, layers = 0;
    int proj = 0;  // the final projection's width (mel channels); 0: none (the encoder)
    bool tfused = false, att_f32 = false;  // the handle's
    // each layer's wide_scores, bit l for layer l (set_wide); a stack deeper
    // than 64 layers shares bit 63 among layers 63 and up, so a wide layer
    // there puts them all on the f32-base form, which is exact for any scores
    uint64_t wide = 0;
    TfSrc src = TfSrc::X;
    bool masked = false;    // lengths given
    bool device_T = false;  // N is the capacity, the frame count a device word
    bool ragged = false;    // per-utterance rows
    int B = 0, N = 0;

    void set_wide(int l) { wide |= uint64_t{1} << (l < 63 ? l : 63); }
    bool wide_scores(int l) const { return (wide >> (l < 63 ? l : 63)) & 1u; }
};

// One-launch layers (transformer_layer.hip) for this stack: the split-f16
// transformer path on a supported (H, heads).  M2_TF_LAYER=0 keeps the
// three-launch layers (A/B comparisons, tests).
inline bool tf_one_launch(const TfCall& c, const Switches& s) {
    return s.tf_layer && c.tfused && !c.att_f32 && c.layers > 0 && tfl_supported(c.H, c.heads);
}
// Each post-attention kernel also runs the next layer's LN1 -> QKV on its row
// tile, one launch per layer fewer; results are identical to the separate
// launches (same fp32 y into the same LayerNorm / GEMM code).  M2_TF_CHAIN=0:
// separate ln_gemm launches (A/B).
inline bool tf_chained(const TfCall& c, const Switches& s) {
    return s.tf_chain && c.tfused && tf_post_next_supported(c.H, 3 * c.H);
}
// The form a call takes; a stack without layers reports what its layers would.
inline int tf_form(const TfCall& c, const Switches& s) {
    if (tf_one_launch(c, s)) return 3;
    if (!c.tfused) return 0;
    return tf_chained(c, s) ? 2 : 1;
}
// The last one-launch layer runs the final projection.
inline bool tf_one_launch_projects(const TfCall& c, const Switches& s) {
    return tf_one_launch(c, s) && c.proj > 0 && tfl_proj_supported(c.H, c.proj);
}

struct TfError {
    int32_t code = M2_OK;
    const char* text = nullptr;
};
// What a non-empty call needs of its stack: a device frame count (N is the
// capacity of a speculative launch) the one-launch layers with the projection
// fused into the last one, per-utterance rows the one-launch layers.
inline TfError tf_call_error(const TfCall& c, const Switches& s) {
    if (c.device_T && !tf_one_launch_projects(c, s))
        return {M2_E_ARG, "mel decoder: a device frame count needs the one-launch layers"};
    if (c.ragged && !tf_one_launch(c, s))
        return {M2_E_SHAPE, "mel decoder: per-utterance frame counts need the one-launch layers "
                            "(hidden_dim 32 / 64 / 96 with 2 heads, M2_TF_LAYER not 0)"};
    return {};
}

enum class TfKind : uint8_t {
    EmbedPe, EmbedLnGemm, LrExpand, ExpandLnGemm, LnGemm, Linear, Attention, PostAttn, PostAttnNext, TflFirst, TflLayer,
    FinalLnGemm, FinalLinear
};
constexpr const char* kTfKindNames[] = {"embed_pe", "embed_ln_gemm", "lr_expand", "expand_ln_gemm", "ln_gemm",
                                        "linear", "attention", "post_attn", "post_attn_next", "tfl_first",
                                        "tfl_layer", "final_ln_gemm", "final_linear"};

struct TfRow {
    TfKind kind;
    int layer = 0;
    int next = 0;  // post_attn_next / tfl_layer: 1 the next layer's LN1 -> QKV, 2 the final LN -> projection
    int op = 0;    // linear: 0 LN1 -> QKV, 1 out, 2 LN2 -> FF1, 3 FF2
    int rb = 0, qs2 = 0, waves = 0, grid = 0, threads = 0;  // 0: not this kind's
};

struct TfPlan {
    TfCall call;
    int form = 0;
    TfError error;
    bool projected = false;  // the last layer runs the final projection
    std::vector<TfRow> rows;
    int print(char* out, size_t cap) const;
};

inline TfPlan plan_transformer(const TfCall& c, const Switches& s) {
    TfPlan p;
    p.call = c;
    p.form = tf_form(c, s);
    if (c.B <= 0 || c.N <= 0) return p;  // an empty call launches nothing (and is not an error)
    p.error = tf_call_error(c, s);
    if (p.error.code) return p;
    const int H = c.H, n = c.layers, R = c.B * c.N;
    p.rows.reserve((p.form == 0 ? 5 : 3) * (size_t)n + 2);
    auto row = [&](TfKind k, int layer) -> TfRow& {
        p.rows.push_back(TfRow{k, layer});
        return p.rows.back();
    };
    auto gemm = [&](TfKind k, int layer, int next = 0) {  // a 32-row-tile launch of transformer_fused.hip
        TfRow& r = row(k, layer);
        r.next = next;
        r.waves = tf_waves(R, s);
        r.grid = tf_grid(R);
        r.threads = 64 * r.waves;
    };
    auto ending = [&] {
        if (c.proj <= 0 || p.projected) return;
        if (c.tfused && tf_ln_gemm_supported(H, c.proj)) gemm(TfKind::FinalLnGemm, n);
        else row(TfKind::FinalLinear, n);
    };
    if (p.form == 3) {
        TfRow& f = row(TfKind::TflFirst, 0);
        f.rb = tfl_first_rb(c.B, c.N, c.masked, s);
        f.grid = tfl_grid(c.B, c.N, f.rb);
        f.threads = tfl::fk_nw(f.rb) * 64;
        for (int l = 0; l < n; ++l) {
            TfRow& r = row(TfKind::TflLayer, l);
            r.next = l + 1 < n ? 1 : (tf_one_launch_projects(c, s) ? 2 : 0);
            r.rb = tfl_layer_rb(c.B, c.N, c.masked, s);
            r.qs2 = tfl_qs2(H, c.heads, c.masked, c.wide_scores(l), s);
            r.grid = tfl_grid(c.B, c.N, r.rb);
            r.threads = tfl::kWaves * 64;
            p.projected = r.next == 2;
        }
        ending();
        return p;
    }
    // the first layer's input rows: built by its LN1 -> QKV launch where the
    // chain is on and the stack has a layer, else by a launch of their own
    const bool chain = p.form == 2;
    const bool first_fused = chain && n > 0 && tf_src_fused_supported(H, 3 * H);
    if (c.src != TfSrc::X) {
        const bool embed = c.src == TfSrc::Embed;
        if (first_fused) gemm(embed ? TfKind::EmbedLnGemm : TfKind::ExpandLnGemm, 0);
        else row(embed ? TfKind::EmbedPe : TfKind::LrExpand, 0);
    }
    if (chain && n > 0 && !(first_fused && c.src != TfSrc::X)) gemm(TfKind::LnGemm, 0);
    for (int l = 0; l < n; ++l) {
        if (p.form == 0) {
            row(TfKind::Linear, l).op = 0;
            row(TfKind::Attention, l);
            for (int op = 1; op < 4; ++op) row(TfKind::Linear, l).op = op;
            continue;
        }
        if (!chain) gemm(TfKind::LnGemm, l);
        row(TfKind::Attention, l);
        if (chain && l + 1 < n) {
            gemm(TfKind::PostAttnNext, l, 1);
        } else if (chain && c.proj > 0 && tf_post_next_supported(H, c.proj)) {
            gemm(TfKind::PostAttnNext, l, 2);
            p.projected = true;
        } else {
            gemm(TfKind::PostAttn, l);
        }
    }
    ending();
    return p;
}

inline int TfPlan::print(char* out, size_t cap) const {
    size_t n = 0;
    auto put = [&](const char* fmt, auto... a) {
        const int k = std::snprintf(out && n < cap ? out + n : nullptr, out && n < cap ? cap - n : 0, fmt, a...);
        if (k > 0) n += (size_t)k;
    };
    static constexpr const char* kSrc[] = {"x", "embed", "expand"};
    put("%s form=%d H=%d heads=%d layers=%d B=%d N=%d src=%s masked=%d devT=%d ragged=%d projected=%d",
        call.decoder ? "dec" : "enc", form, call.H, call.heads, call.layers, call.B, call.N, kSrc[(int)call.src],
        (int)call.masked, (int)call.device_T, (int)call.ragged, (int)projected);
    if (error.code) put(" error=\"%s\"", error.text);
    for (const TfRow& r : rows) {
        const char* name = kTfKindNames[(int)r.kind];
        switch (r.kind) {
            case TfKind::EmbedPe:
            case TfKind::LrExpand:
            case TfKind::FinalLinear: put(" %s", name); break;
            case TfKind::Attention: put(" %s%d", name, r.layer); break;
            case TfKind::Linear: put(" %s%d[op=%d]", name, r.layer, r.op); break;
            case TfKind::FinalLnGemm: put(" %s[waves=%d grid=%d thr=%d]", name, r.waves, r.grid, r.threads); break;
            case TfKind::PostAttnNext:
                put(" %s%d[next=%d waves=%d grid=%d thr=%d]", name, r.layer, r.next, r.waves, r.grid, r.threads);
                break;
            case TfKind::TflFirst: put(" %s%d[rb=%d grid=%d thr=%d]", name, r.layer, r.rb, r.grid, r.threads); break;
            case TfKind::TflLayer:
                put(" %s%d[next=%d rb=%d qs2=%d grid=%d thr=%d]", name, r.layer, r.next, r.rb, r.qs2, r.grid, r.threads);
                break;
            default: put(" %s%d[waves=%d grid=%d thr=%d]", name, r.layer, r.waves, r.grid, r.threads); break;
        }
    }
    return (int)n;
}

}  // namespace m2
