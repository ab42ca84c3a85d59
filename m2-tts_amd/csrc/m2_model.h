// The model handle, its weight table, and the host-only plan that
// m2_model_create (m2_model.hip) makes from one host copy of the weights.
#pragma once
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "m2_common.h"
#include "vocoder_fused.h"

namespace m2 {

constexpr int kRates[4] = {4, 4, 2, 2};  // tts_model.py:244

// Weight table in M2TTSModel.state_dict() order (tts_model.py:303-343).
struct WSpec {
    std::string name;
    int64_t numel;
    bool is_int64;
};
std::vector<WSpec> weight_table(const m2_config& c);
bool config_ok(const m2_config* c);

}  // namespace m2

struct m2_layer_w {
    const float *qkv_w, *out_w, *out_b, *ff1_w, *ff1_b, *ff2_w, *ff2_b, *n1_w, *n1_b, *n2_w, *n2_b;
    // B-fragment packs for the fused layer kernels (transformer_fused.hip)
    const float *qkv_p = nullptr, *out_p = nullptr, *ff1_p = nullptr, *ff2_p = nullptr;
    // the layer's attention scores (log2 units, scale folded) may leave the
    // f16 range: its one-launch form keeps the softmax base in f32 (TflLayer)
    bool wide_scores = false;
};

struct m2_model {
    m2_config cfg{};
    float* buf = nullptr;
    std::vector<m2_layer_w> enc, dec;
    const float *emb = nullptr, *pe = nullptr, *enc_nw = nullptr, *enc_nb = nullptr;
    const float* dur[10] = {};  // w1,b1,alpha1,beta1, w2,b2,alpha2,beta2, proj_w, proj_b
    // the duration convs' split-f16 fragments, used on the inference path
    // (fused final LayerNorm) when the static range bound allows (dur_split)
    const float* dur_split_w[2] = {};
    bool dur_split = false;
    const float *dec_nw = nullptr, *dec_nb = nullptr, *mel_w = nullptr, *mel_b = nullptr;
    const float* mel_p = nullptr;  // packed mel projection (fused path)
    bool tfused = false;           // transformer layers on ln_gemm + attention + post_attn
    const float *vin_w = nullptr, *vin_b = nullptr, *vout_w = nullptr, *vout_b = nullptr;
    const float *up_w[4] = {}, *up_b[4] = {};
    const float *rb_w1[4] = {}, *rb_b1[4] = {}, *rb_w2[4] = {}, *rb_b2[4] = {};
    // fused vocoder: packed weights
    float* vbuf = nullptr;
    m2::VocW vw{};
    bool fused = false;
    // split-f16 vocoder (vocoder_x3.hip): packed hi/lo weights; preferred when supported
    void* xbuf = nullptr;
    m2::VocX vx{};
    bool x3 = false;
    void* tbuf = nullptr;  // pipelined tail pack (stage1: vx.tp / vx.tpb, stage2: vx.tp2 / vx.tp2b)
    bool tailp = false;
    void* mbuf = nullptr;  // pipelined stage1 mid pack (vx.mp / vx.mpb)
    bool midp = false;
    bool x3_packed = false;  // split-f16 packs exist (m2_vocoder_select can switch x3 on/off)
    // streamed vocoder (m2_vocoder_set_chunking): chunks of chunk_frames mel
    // frames, each computed over a window widened by kVocHalo frames per side
    int chunk_frames = 0;
    // split-f16 range: non-finite-audio flag (host-mapped, vx.rflag is its
    // device address), what a raised flag does (m2_set_range_policy), and the
    // exact-f32 attention for weights whose q/k/v bound leaves the f16 range
    int32_t* rflag_host = nullptr;
    // range policy 1 on the fused vocoders: two device flag words used by
    // alternate calls (rseq parity) - the split kernels raise the call's word,
    // the exact-f32 redo kernels run only when it is raised, and the next
    // call's head kernel zeroes it
    int* rflag_dev = nullptr;
    mutable unsigned rseq = 0;
    // policy 1 on the pipelined tails: the tail's in-launch local redo
    // instead of the guarded exact-f32 launch (vocoder_redo.h); device copy
    const m2::VocRedoW* redo_w = nullptr;
    // the same table for the ragged entry points' end fix-up (vocoder_ragged.hip):
    // present on every fused vocoder, also where no tail redo is wired
    const m2::VocRedoW* ragged_w = nullptr;
    int range_policy = 0;
    // one-launch transformer layers: work-queue counters and the launch
    // sequence whose parity picks their set (one stream per model)
    unsigned* tflq = nullptr;
    mutable unsigned tfl_seq = 0;
    // device-T path: the count kernel's ticket word (after the queue words in
    // tflq) and the host-mapped [seq, T] pair the back half's first launch
    // posts (m2_frames_wait)
    unsigned* cnt_ticket = nullptr;
    int32_t* fpost_host = nullptr;
    int32_t* fpost_dev = nullptr;
    mutable int32_t fpost_seq = 0;
    bool att_f32 = false;
    // measurement: per m2_vocoder call, an event pair around each fused kernel
    mutable std::vector<hipEvent_t> prof_begin, prof_end;  // [call][kernel]
    mutable int prof_calls = 0;
    uint32_t prof_mask = ~0u;  // which kernels get an event pair (m2_profile_select)
    int prof_stride = 1;       // record on every prof_stride-th call (m2_profile_stride)
    mutable long prof_seen = 0;
};

namespace m2 {

// ---------------------------------------------------------------------------
// The plan: every decision and every packed buffer of a handle, computed on
// the host from one copy of the raw weights.  None of these functions makes a
// HIP call (tools/plan_check.cpp runs them without a GPU).

// m2_model::buf in floats, 64-float aligned carves: every fp32 weight
// verbatim (off[i]; the raw span, [0, bn_off)), then the derived span - 2 x
// (alpha, beta) of the BatchNorm inference form, the duration conv weights in
// B-fragment order and as split-f16 fragments, and the fused transformer
// layers' packs (8 H^2 per layer + the mel projection; reserved always).
struct BufLayout {
    std::vector<size_t> off;
    size_t bn_off, dw_off, dws_off, tf_off, total;
};
BufLayout buf_layout(const std::vector<WSpec>& table, const m2_config& c);

// The raw span on the host, addressed by state_dict name.
struct HostWeights {
    const std::vector<WSpec>& table;
    const BufLayout& lay;
    std::vector<float> raw;
    struct View {
        const float* p;
        size_t n;
        const float* begin() const { return p; }
        const float* end() const { return p + n; }
        float operator[](size_t i) const { return p[i]; }
    };
    int index(const std::string& name) const;
    View operator()(const std::string& name) const;
};

// Parts appended at Align-element alignment (gaps zero), each with the pointer
// slot that receives its device address once the buffer is uploaded.
template <typename T, size_t Align, typename P = const T*>
struct PackList {
    std::vector<T> host;
    std::vector<std::pair<P*, size_t>> slots;
    template <typename V>
    void add(const V& part, P* slot) {
        const size_t at = align_up(host.size(), Align);
        host.resize(at, T(0));
        host.insert(host.end(), part.begin(), part.end());
        slots.push_back({slot, at});
    }
    void patch(T* base) const {
        for (const auto& s : slots) *s.first = reinterpret_cast<P>(base + s.second);
    }
};

struct DurationPlan {
    std::vector<float> bn;     // [alpha1, beta1', alpha2, beta2'] x H
    std::vector<float> pack;   // 2 x 3H^2, exact-f32 B fragments (always written)
    std::vector<float> split;  // 2 x 3H^2, split-f16 fragments (zeros for a layer outside the f16 range)
    bool dur_split;
};
DurationPlan plan_duration(const HostWeights& w, const m2_config& c);

struct TransformerPlan {
    // per layer (encoder, then decoder) qkv, out, ffn1, ffn2, then the mel
    // projection, back to back; packing stops at the first weight outside the
    // f16 range (at[] holds the offsets of the packs made up to there)
    std::vector<float> packs;
    std::vector<size_t> at;
    std::vector<char> wide_scores;  // per layer
    bool tfused, att_f32;
};
TransformerPlan plan_transformer(const HostWeights& w, const m2_config& c, const Switches& s);

// A pipelined kernel's pack: the u16 weights, then its fp32 bias table as u16
// pairs from bias_at on; empty when the kernel is not used.
struct PipePlan {
    std::vector<uint16_t> buf;
    size_t bias_at = 0;
};

// Filled in place: the slots of its packs point into vw / vx / hc*_at.
struct VocoderPlan {
    bool fused = false;  // the exact-f32 MFMA family (f32, vw)
    // the split-f16 family (split, vx; tail and mid only with it): shapes
    // supported, not switched off, every weight inside the f16 range
    bool x3 = false;
    VocW vw{};
    VocX vx{};
    const vx_u32x4 *hcb_at = nullptr, *hce_at = nullptr;  // the composed split head's fp32 tables (u16 pairs)
    PackList<float, 64> f32;
    PackList<uint16_t, 128, const vx_u32x4*> split;
    PipePlan tail, mid;
    VocoderPlan() = default;
    VocoderPlan(const VocoderPlan&) = delete;
};
void plan_vocoder(const HostWeights& w, const m2_config& c, const Switches& s, VocoderPlan* out);

}  // namespace m2
