// The model handle: weight table, the host-only plan (decisions and packed
// buffers, no HIP call) and m2_model_create / m2_model_destroy, which stage
// the weights, read them back once, plan and upload.
#include "m2_model.h"

#include <algorithm>
#include <cmath>

#include "transformer_fused.h"
#include "transformer_layer.h"

namespace m2 {

static void add_layer(std::vector<WSpec>& t, const std::string& p, int64_t H) {
    t.push_back({p + ".self_attn.qkv.weight", 3 * H * H, false});
    t.push_back({p + ".self_attn.out_proj.weight", H * H, false});
    t.push_back({p + ".self_attn.out_proj.bias", H, false});
    t.push_back({p + ".ffn.linear1.weight", 2 * H * H, false});
    t.push_back({p + ".ffn.linear1.bias", 2 * H, false});
    t.push_back({p + ".ffn.linear2.weight", 2 * H * H, false});
    t.push_back({p + ".ffn.linear2.bias", H, false});
    t.push_back({p + ".norm1.weight", H, false});
    t.push_back({p + ".norm1.bias", H, false});
    t.push_back({p + ".norm2.weight", H, false});
    t.push_back({p + ".norm2.bias", H, false});
}

std::vector<WSpec> weight_table(const m2_config& c) {
    std::vector<WSpec> t;
    const int64_t H = c.hidden_dim, M = c.mel_channels, C = c.vocoder_channels;
    t.push_back({"text_encoder.embedding.weight", (int64_t)c.vocab_size * H, false});
    t.push_back({"text_encoder.pos_encoding.pe", (int64_t)c.max_positions * H, false});
    for (int i = 0; i < c.text_encoder_layers; ++i) add_layer(t, "text_encoder.layers." + std::to_string(i), H);
    t.push_back({"text_encoder.norm.weight", H, false});
    t.push_back({"text_encoder.norm.bias", H, false});
    for (int j = 0; j < 2; ++j) {
        const std::string p = "duration_predictor.predictor.conv_layers." + std::to_string(j);
        t.push_back({p + ".conv.weight", H * H * 3, false});
        t.push_back({p + ".conv.bias", H, false});
        t.push_back({p + ".norm.weight", H, false});
        t.push_back({p + ".norm.bias", H, false});
        t.push_back({p + ".norm.running_mean", H, false});
        t.push_back({p + ".norm.running_var", H, false});
        t.push_back({p + ".norm.num_batches_tracked", 1, true});
    }
    t.push_back({"duration_predictor.predictor.projection.weight", H, false});
    t.push_back({"duration_predictor.predictor.projection.bias", 1, false});
    for (int i = 0; i < c.decoder_layers; ++i) add_layer(t, "decoder.layers." + std::to_string(i), H);
    t.push_back({"decoder.norm.weight", H, false});
    t.push_back({"decoder.norm.bias", H, false});
    t.push_back({"decoder.mel_projection.weight", M * H, false});
    t.push_back({"decoder.mel_projection.bias", M, false});
    t.push_back({"vocoder.input_conv.weight", C * M * 3, false});
    t.push_back({"vocoder.input_conv.bias", C, false});
    int64_t ch = C;
    for (int k = 0; k < 4; ++k) {
        const std::string p = "vocoder.upsamples." + std::to_string(k);
        t.push_back({p + ".weight", ch * (ch / 2) * 2 * kRates[k], false});
        t.push_back({p + ".bias", ch / 2, false});
        ch /= 2;
    }
    ch = C;
    for (int k = 0; k < 4; ++k) {
        ch /= 2;
        const std::string p = "vocoder.resblocks." + std::to_string(k);
        t.push_back({p + ".conv1.weight", ch * ch * 3, false});
        t.push_back({p + ".conv1.bias", ch, false});
        t.push_back({p + ".conv2.weight", ch * ch * 3, false});
        t.push_back({p + ".conv2.bias", ch, false});
    }
    t.push_back({"vocoder.output_conv.weight", ch * 3, false});
    t.push_back({"vocoder.output_conv.bias", 1, false});
    return t;
}

bool config_ok(const m2_config* c) {
    if (!c) return false;
    const bool pos = c->vocab_size > 0 && c->hidden_dim > 0 && c->mel_channels > 0 &&
                     c->text_encoder_layers >= 0 && c->decoder_layers >= 0 && c->num_heads > 0 &&
                     c->vocoder_channels >= 16 && c->max_positions > 0;
    return pos && c->hidden_dim % c->num_heads == 0 && c->vocoder_channels % 16 == 0;
}

BufLayout buf_layout(const std::vector<WSpec>& table, const m2_config& c) {
    const size_t H = c.hidden_dim;
    BufLayout l;
    l.off.assign(table.size(), 0);
    size_t total = 0;
    auto carve = [&](size_t n) {
        const size_t at = total = align_up(total, 64);
        total += n;
        return at;
    };
    for (size_t i = 0; i < table.size(); ++i)
        if (!table[i].is_int64) l.off[i] = carve((size_t)table[i].numel);
    l.bn_off = carve(4 * H);
    l.dw_off = carve(2 * 3 * H * H);
    l.dws_off = carve(2 * 3 * H * H);
    l.tf_off = carve((size_t)(c.text_encoder_layers + c.decoder_layers) * 8 * H * H + (size_t)c.mel_channels * H);
    l.total = total;
    return l;
}

int HostWeights::index(const std::string& name) const {
    for (size_t i = 0; i < table.size(); ++i)
        if (table[i].name == name) return (int)i;
    return -1;
}

HostWeights::View HostWeights::operator()(const std::string& name) const {
    const int i = index(name);
    return View{raw.data() + lay.off[i], (size_t)table[i].numel};
}

static std::vector<std::string> layer_prefixes(const m2_config& c) {
    std::vector<std::string> p;
    for (int i = 0; i < c.text_encoder_layers; ++i) p.push_back("text_encoder.layers." + std::to_string(i));
    for (int i = 0; i < c.decoder_layers; ++i) p.push_back("decoder.layers." + std::to_string(i));
    return p;
}

static double amax(HostWeights::View v) {
    double a = 0.0;
    for (float x : v) a = std::max(a, (double)std::fabs(x));
    return a;
}

// sum_k |row[k]| in double, in k order; its maximum over the N rows of W[N][K]
static double row_abs(const float* row, int K) {
    double sum = 0.0;
    for (int k = 0; k < K; ++k) sum += std::fabs(row[k]);
    return sum;
}
static double max_row_abs(const float* W, int N, int K) {
    double best = 0.0;
    for (int r = 0; r < N; ++r) best = std::max(best, row_abs(W + (size_t)r * K, K));
    return best;
}

DurationPlan plan_duration(const HostWeights& w, const m2_config& c) {
    const int H = c.hidden_dim;
    const std::string conv = "duration_predictor.predictor.conv_layers.";
    DurationPlan d;
    // BatchNorm1d eval: alpha = gamma / sqrt(var + eps), beta' = beta - mean * alpha
    // (ATen batch_norm_cpu_collect_linear_and_constant_terms, fp32).
    d.bn.resize(4 * (size_t)H);
    for (int j = 0; j < 2; ++j) {
        const std::string p = conv + std::to_string(j) + ".norm.";
        const auto bnw = w(p + "weight"), bnb = w(p + "bias"), bnm = w(p + "running_mean"), bnv = w(p + "running_var");
        for (int ch = 0; ch < H; ++ch) {
            const float invstd = 1.0f / std::sqrt(bnv[ch] + 1e-5f);
            const float a = invstd * bnw[ch];
            d.bn[(2 * j) * H + ch] = a;
            d.bn[(2 * j + 1) * H + ch] = bnb[ch] - bnm[ch] * a;
        }
    }
    // Duration convs: W[co][ci][tap] -> GEMM B matrix [co][tap*H + ci] -> B-fragment order
    // (exact-f32 MFMA) and split-f16 hi/lo fragments (v_mfma_f32_16x16x32_f16).
    d.pack.assign(2 * 3 * (size_t)H * H, 0.f);
    d.split.assign(2 * 3 * (size_t)H * H, 0.f);
    bool dsplit = true;
    double dconv_rows[2];  // max over co of sum_{ci, tap} |W[co][ci][tap]|
    for (int j = 0; j < 2; ++j) {
        const auto cw = w(conv + std::to_string(j) + ".conv.weight");
        std::vector<float> wt((size_t)3 * H * H);
        for (int co = 0; co < H; ++co)
            for (int ci = 0; ci < H; ++ci)
                for (int k = 0; k < 3; ++k) wt[(size_t)co * 3 * H + k * H + ci] = cw[((size_t)co * H + ci) * 3 + k];
        const std::vector<float> pk = pack_bfrag(wt.data(), H, 3 * H);
        std::copy(pk.begin(), pk.end(), d.pack.begin() + (size_t)j * 3 * H * H);
        std::vector<float> pks;
        if (!pack_bfrag_split(wt.data(), H, 3 * H, &pks)) dsplit = false;
        else std::copy(pks.begin(), pks.end(), d.split.begin() + (size_t)j * 3 * H * H);
        dconv_rows[j] = max_row_abs(wt.data(), H, 3 * H);
    }
    // Split-f16 range of the duration convs on the inference path, where their
    // input is the encoder's final LayerNorm (|LN| <= sqrt(H-1) max|gamma| +
    // max|beta|) and conv2's input is BN(conv1) after ReLU (<= max|alpha| (row
    // sum |W1| x that + max|b1|) + max|beta'|): checked once here against half
    // the f16 range, as the transformer's bound below; outside it (or with a
    // weight outside the f16 range) the exact-f32 MFMA convs stay.
    const double ga = amax(w("text_encoder.norm.weight")), ba = amax(w("text_encoder.norm.bias"));
    const double b1a = amax(w(conv + "0.conv.bias"));
    const double a1a = amax({d.bn.data(), (size_t)H}), c1a = amax({d.bn.data() + H, (size_t)H});
    const double x0 = std::sqrt((double)std::max(H - 1, 1)) * ga + ba;
    const double x1 = a1a * (dconv_rows[0] * x0 + b1a) + c1a;
    d.dur_split = dsplit && x0 < 32768.0 && x1 < 32768.0;
    return d;
}

TransformerPlan plan_transformer(const HostWeights& w, const m2_config& c, const Switches& s) {
    const int H = c.hidden_dim;
    const std::vector<std::string> layers = layer_prefixes(c);
    TransformerPlan t;
    // Fused transformer layers: pack qkv / out / ffn / mel-projection weights
    // in B-fragment order (M2_TF_UNFUSED=1 keeps the five-linear layer); a
    // weight outside the f16 range keeps the fp32 five-linear layers too.
    t.tfused = tf_fused_supported(H, 3 * H) && tf_fused_supported(H, c.mel_channels) && !s.tf_unfused;
    auto pack = [&](const std::string& n, int N, int K) {
        std::vector<float> pk;
        if (!t.tfused || !(t.tfused = pack_bfrag_split(w(n).p, N, K, &pk))) return;  // false: |w| >= 65504
        t.at.push_back(t.packs.size());
        t.packs.insert(t.packs.end(), pk.begin(), pk.end());
    };
    for (const std::string& p : layers) {
        pack(p + ".self_attn.qkv.weight", 3 * H, H);
        pack(p + ".self_attn.out_proj.weight", H, H);
        pack(p + ".ffn.linear1.weight", 2 * H, H);
        pack(p + ".ffn.linear2.weight", H, 2 * H);
    }
    pack("decoder.mel_projection.weight", c.mel_channels, H);
    // Split-f16 range of the transformer.  Its split operands are LayerNorm
    // outputs (|x^| <= sqrt(H-1) for a normalised row, so |LN| <= sqrt(H-1)
    // max|gamma| + max|beta|), q/k/v = W_qkv LN1 (<= max row sum |W| x that),
    // attention outputs (convex combinations of v) and ReLU(FFN1(LN2)) - all
    // bounded by the weights, so the check is made once, here: past half the
    // f16 range the layers use the fp32 linears and the exact-f32 attention.
    auto ln_bound = [&](const std::string& p) {
        return std::sqrt((double)std::max(H - 1, 1)) * amax(w(p + ".weight")) + amax(w(p + ".bias"));
    };
    // scores in log2 units, |q.k| scale log2(e) <= sum over a head's dims of
    // |q_d| |k_d| (each bounded by its row sum of |W_qkv| x the LN1 bound)
    // x scale log2(e): the head_dim-48 wave-specialised attention holds its
    // softmax base m (<= the largest score) as an f16 hi / lo pair, finite
    // while |m| < 65520, so a layer whose bound reaches the f16 maximum
    // runs the f32-base form (m2_layer_w::wide_scores; the seeded stage2
    // weights bound at ~3.5e4)
    const int heads = c.num_heads, hd = H / std::max(heads, 1);
    const double sl2 = 1.0 / std::sqrt((double)hd) * 1.4426950408889634;
    double worst = 0.0;
    for (const std::string& p : layers) {
        const double b1 = ln_bound(p + ".norm1"), b2 = ln_bound(p + ".norm2");
        const float* wq = w(p + ".self_attn.qkv.weight").p;
        const double qkv = max_row_abs(wq, 3 * H, H) * b1;
        // rows of W_qkv: the reference's reshape (3, heads, head_dim)
        auto rs = [&](int r) { return row_abs(wq + (size_t)r * H, H) * b1; };
        double sb = 0.0;
        for (int h = 0; h < heads; ++h) {
            double acc = 0.0;
            for (int d = 0; d < hd; ++d) acc += rs(h * hd + d) * rs(H + h * hd + d);
            sb = std::max(sb, acc * sl2);
        }
        t.wide_scores.push_back(!(sb < 65504.0));
        const double hid = max_row_abs(w(p + ".ffn.linear1.weight").p, 2 * H, H) * b2 + amax(w(p + ".ffn.linear1.bias"));
        worst = std::max(worst, std::max(std::max(b1, b2), std::max(qkv, hid)));
    }
    if (c.decoder_layers > 0) worst = std::max(worst, ln_bound("decoder.norm"));
    // M2_ATT_F32=1 asks for the same path at handle creation, as M2_TF_UNFUSED
    // does for the linears: fp32 linears and attention_kernel<HD>
    t.att_f32 = !(worst < 32768.0) || s.att_f32;
    if (t.att_f32) t.tfused = false;
    return t;
}

// The stage1 / stage2 vocoder shapes: the ones with a composed head and a pipelined tail.
static bool is_s1(const m2_config& c) { return c.mel_channels == 64 && c.vocoder_channels == 128; }
static bool is_s2(const m2_config& c) { return c.mel_channels == 80 && c.vocoder_channels == 256; }

// upsamples.k's weight and bias, resblocks.k's conv1 and conv2 weight and bias
struct StageW {
    HostWeights::View wt, bt, w1, b1, w2, b2;
};
static StageW stage_w(const HostWeights& w, int k) {
    const std::string u = "vocoder.upsamples." + std::to_string(k), r = "vocoder.resblocks." + std::to_string(k);
    return {w(u + ".weight"),     w(u + ".bias"),         w(r + ".conv1.weight"),
            w(r + ".conv1.bias"), w(r + ".conv2.weight"), w(r + ".conv2.bias")};
}

// input_conv composed into ConvT1 (stage1 / stage2 shapes) at MP padded mel channels
static bool head_comp(const HostWeights& w, const m2_config& c, int MP, std::vector<uint16_t>* hw,
                      std::vector<float>* hb, std::vector<float>* he, bool* hok) {
    const StageW g = stage_w(w, 0);
    return (is_s1(c) || is_s2(c)) &&
           pack_x3_head_comp(w("vocoder.input_conv.weight").p, w("vocoder.input_conv.bias").p, g.wt.p, g.bt.p,
                             c.mel_channels, MP, c.vocoder_channels, hw, hb, he, hok);
}

// Fused vocoder: pack conv / convT weights into MFMA A-fragment order.
static void plan_vocoder_f32(const HostWeights& w, const m2_config& c, VocoderPlan* out) {
    const int M = c.mel_channels, C = c.vocoder_channels;
    VocW& vw = out->vw;
    auto& pk = out->f32;
    const auto wi = w("vocoder.input_conv.weight");
    pk.add(pack_conv3(wi.p, C, M), &vw.wi);
    pk.add(w("vocoder.input_conv.bias"), &vw.bi);
    int ch = C;
    for (int k = 0; k < 4; ++k) {
        const StageW g = stage_w(w, k);
        pk.add(pack_convT(g.wt.p, ch, ch / 2, kRates[k]), &vw.wt[k]);
        pk.add(g.bt, &vw.bt[k]);
        ch /= 2;
        pk.add(pack_conv3(g.w1.p, ch, ch), &vw.w1[k]);
        pk.add(g.b1, &vw.b1[k]);
        pk.add(pack_conv3(g.w2.p, ch, ch), &vw.w2[k]);
        pk.add(g.b2, &vw.b2[k]);
        if (k == 3 && ch == 8 && kRates[3] == 2) {  // the two-phase forms of the last stage
            pk.add(pack_convT2_paired(g.wt.p, 2 * ch), &vw.wt4p);
            pk.add(pack_conv3_2p(g.w1.p), &vw.w1p);
            pk.add(pack_conv3_2p(g.w2.p), &vw.w2p);
        }
    }
    // the exact-f32 head's composed input conv o ConvT1 (hok, the f16 range of the split weights: no matter here)
    std::vector<uint16_t> hw_unused;
    std::vector<float> hb, he;
    bool hok = true;
    if (head_comp(w, c, M, &hw_unused, &hb, &he, &hok)) {
        pk.add(pack_f32_head_comp(wi.p, w("vocoder.upsamples.0.weight").p, M, C), &vw.hcw);
        pk.add(hb, &vw.hcb);
        pk.add(he, &vw.hce);
    }
}

// Split-f16 packs; false when a weight is outside the f16 range.
static bool plan_vocoder_split(const HostWeights& w, const m2_config& c, VocoderPlan* out) {
    const int M = c.mel_channels, C = c.vocoder_channels;
    bool ok = true;
    VocX& vx = out->vx;
    auto& pk = out->split;
    pk.add(pack_x3_conv3(w("vocoder.input_conv.weight").p, C, M, vocoder_x3_mel_pad(M), &ok, false), &vx.wi);
    int ch = C;
    for (int k = 0; k < 4; ++k) {
        const StageW g = stage_w(w, k);
        pk.add(pack_x3_convT(g.wt.p, ch, ch / 2, kRates[k], &ok), &vx.wt[k]);
        ch /= 2;
        pk.add(pack_x3_conv3(g.w1.p, ch, ch, ch, &ok, false), &vx.w1[k]);
        pk.add(pack_x3_conv3(g.w2.p, ch, ch, ch, &ok, true), &vx.w2[k]);
    }
    // stage1 head: input_conv composed into ConvT1 (fp32 bias / edge
    // tables ride in the same buffer as u16 pairs)
    std::vector<uint16_t> hw;
    std::vector<float> hb, he;
    bool hok = true;
    if (head_comp(w, c, vocoder_x3_mel_pad(M), &hw, &hb, &he, &hok) && hok) {
        auto as_u16 = [](const std::vector<float>& f) {
            std::vector<uint16_t> u(f.size() * 2);
            std::memcpy(u.data(), f.data(), f.size() * sizeof(float));
            return u;
        };
        pk.add(hw, &vx.hc);
        pk.add(as_u16(hb), &out->hcb_at);
        pk.add(as_u16(he), &out->hce_at);
    }
    return ok;
}

// pack(src, &weights, &bias, &range_ok) -> the kernel's one buffer (none when it cannot be used)
template <typename Src, typename Pack>
static PipePlan pipe_plan(const Src& src, Pack pack) {
    PipePlan p;
    std::vector<float> pb;
    bool rok = true;
    if (!(pack(src, &p.buf, &pb, &rok) && rok)) return PipePlan{};
    p.bias_at = p.buf.size();
    p.buf.resize(p.bias_at + 2 * pb.size());
    std::memcpy(p.buf.data() + p.bias_at, pb.data(), pb.size() * sizeof(float));
    return p;
}

void plan_vocoder(const HostWeights& w, const m2_config& c, const Switches& s, VocoderPlan* out) {
    const int M = c.mel_channels, C = c.vocoder_channels;
    out->fused = vocoder_fused_supported(M, C) && !s.voc_perlayer;
    if (!out->fused) return;
    plan_vocoder_f32(w, c, out);
    // Split-f16 packs: the default path when the shapes are supported and every
    // weight is inside the f16 range - one outside it drops the whole split
    // family (M2_VOC_F32=1 keeps the exact-f32 MFMA).
    out->x3 = vocoder_x3_supported(M, C) && !s.voc_f32 && plan_vocoder_split(w, c, out);
    if (!out->x3) {
        out->split = {};
        return;
    }
    const StageW g1 = stage_w(w, 1), g2 = stage_w(w, 2), g3 = stage_w(w, 3);
    // stage1 / stage2: the last two upsampling stages as one pipelined kernel
    // (M2_VOC_TAIL_X3=1 keeps the x3 tail kernel).
    if ((is_s1(c) || is_s2(c)) && !s.voc_tail_x3) {
        const TailpSrc src{g2.wt.p, g2.bt.p, g2.w1.p, g2.b1.p, g2.w2.p, g2.b2.p, g3.wt.p, g3.bt.p, g3.w1.p, g3.b1.p,
                           g3.w2.p, g3.b2.p, w("vocoder.output_conv.weight").p, w("vocoder.output_conv.bias").p};
        out->tail = pipe_plan(src, is_s2(c) ? pack_tailp2 : pack_tailp);
    }
    // stage1: the second upsampling stage as one pipelined kernel
    // (M2_VOC_MID_X3=1 keeps the x3 mid kernel).
    if (is_s1(c) && !s.voc_mid_x3)
        out->mid = pipe_plan(MidpSrc{g1.wt.p, g1.bt.p, g1.w1.p, g1.b1.p, g1.w2.p, g1.b2.p}, pack_midp);
}

}  // namespace m2

using namespace m2;

extern "C" {

int32_t m2_weight_count(const m2_config* cfg) {
    if (!config_ok(cfg)) return fail(M2_E_ARG, "m2_weight_count: invalid config");
    return (int32_t)weight_table(*cfg).size();
}

int32_t m2_weight_name(const m2_config* cfg, int32_t index, char* buf, int32_t buflen) {
    if (!config_ok(cfg) || !buf || buflen <= 0) return fail(M2_E_ARG, "m2_weight_name: bad argument");
    const auto t = weight_table(*cfg);
    if (index < 0 || index >= (int32_t)t.size()) return fail(M2_E_ARG, "m2_weight_name: index out of range");
    const std::string& n = t[index].name;
    if ((int32_t)n.size() + 1 > buflen) return fail(M2_E_ARG, "m2_weight_name: buffer too small");
    std::memcpy(buf, n.c_str(), n.size() + 1);
    return M2_OK;
}

int64_t m2_weight_numel(const m2_config* cfg, int32_t index) {
    if (!config_ok(cfg)) return fail(M2_E_ARG, "m2_weight_numel: invalid config");
    const auto t = weight_table(*cfg);
    if (index < 0 || index >= (int32_t)t.size()) return fail(M2_E_ARG, "m2_weight_numel: index out of range");
    return t[index].numel;
}

int32_t m2_model_create(const m2_config* cfg, const void* const* weights, int32_t n_weights,
                        void* stream, m2_model** out) {
    reload_switches();  // the developer switches of this handle's creation (m2_common.h)
    M2_CHECK_ARG(config_ok(cfg), "m2_model_create: invalid config");
    M2_CHECK_ARG(weights && out, "m2_model_create: null argument");
    const auto table = weight_table(*cfg);
    if (n_weights != (int32_t)table.size()) return fail(M2_E_WEIGHTS, "m2_model_create: weight count mismatch");
    for (size_t i = 0; i < table.size(); ++i)
        M2_CHECK_ARG(table[i].is_int64 || weights[i] != nullptr, "m2_model_create: null weight pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Switches& s = sw();
    const int H = cfg->hidden_dim;
    const BufLayout lay = buf_layout(table, *cfg);

    auto* m = new m2_model();
    m->cfg = *cfg;
    // From here on every failure leaves through failed(): m2_model_destroy
    // frees whatever exists.  ok(what, call's status) records the first failure
    // (e, where); the steps are chained with &&, so nothing runs after one.
    hipError_t e = hipSuccess;
    const char* where = "";
    auto ok = [&](const char* what, hipError_t r) {
        if (r != hipSuccess) e = r, where = what;
        return r == hipSuccess;
    };
    auto failed = [&] {
        (void)hipStreamSynchronize(st);  // no copy from a host vector of this call still in flight
        m2_model_destroy(m);
        return hip_status(e, where);
    };
    auto copy = [&](const char* what, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
        return ok(what, hipMemcpyAsync(dst, src, bytes, kind, st));
    };
    // one device buffer holding a host vector's elements; none for an empty one
    auto upload = [&](const char* what, auto** dst, const auto& v) {
        const size_t bytes = v.size() * sizeof(v[0]);
        return v.empty() || (ok(what, hipMalloc(dst, bytes)) && copy(what, *dst, v.data(), bytes, hipMemcpyHostToDevice));
    };

    // ---- stage: every fp32 weight verbatim into buf, and that span back to the host, once
    bool g = ok("hipMalloc(model)", hipMalloc(&m->buf, lay.total * sizeof(float)));
    for (size_t i = 0; i < table.size(); ++i)
        g = g && (table[i].is_int64 || copy("hipMemcpyAsync(weight)", m->buf + lay.off[i], weights[i],
                                            table[i].numel * sizeof(float), hipMemcpyDeviceToDevice));
    HostWeights hw{table, lay, std::vector<float>(lay.bn_off)};
    g = g && copy("read weights back", hw.raw.data(), m->buf, lay.bn_off * sizeof(float), hipMemcpyDeviceToHost) &&
        ok("read weights back", hipStreamSynchronize(st));
    if (!g) return failed();

    // ---- plan (host only)
    const DurationPlan dp = plan_duration(hw, *cfg);
    const TransformerPlan tp = plan_transformer(hw, *cfg, s);
    VocoderPlan vp;
    plan_vocoder(hw, *cfg, s, &vp);

    // ---- upload: the derived span of buf in one copy, then one buffer per vocoder family
    std::vector<float> derived(lay.total - lay.bn_off, 0.f);
    auto put = [&](size_t at, const std::vector<float>& v) {
        std::copy(v.begin(), v.end(), derived.begin() + (at - lay.bn_off));
    };
    put(lay.bn_off, dp.bn);
    put(lay.dw_off, dp.pack);
    put(lay.dws_off, dp.split);
    put(lay.tf_off, tp.packs);
    g = copy("upload derived weights", m->buf + lay.bn_off, derived.data(), derived.size() * sizeof(float),
             hipMemcpyHostToDevice) &&
        upload("upload vocoder pack", &m->vbuf, vp.f32.host) && upload("upload x3 pack", &m->xbuf, vp.split.host) &&
        upload("upload tailp pack", &m->tbuf, vp.tail.buf) && upload("upload midp pack", &m->mbuf, vp.mid.buf);
    if (!g) return failed();

    // ---- the handle's pointers and flags
    auto P = [&](const std::string& n) -> const float* { return m->buf + lay.off[hw.index(n)]; };
    m->emb = P("text_encoder.embedding.weight");
    m->pe = P("text_encoder.pos_encoding.pe");
    size_t n_pack = 0;  // tp.at[]: qkv, out, ffn1, ffn2 per layer, then the mel projection
    auto packed = [&] { return n_pack < tp.at.size() ? m->buf + lay.tf_off + tp.at[n_pack++] : nullptr; };
    const std::vector<std::string> layers = layer_prefixes(*cfg);
    for (size_t i = 0; i < layers.size(); ++i) {
        const std::string& p = layers[i];
        m2_layer_w L{P(p + ".self_attn.qkv.weight"), P(p + ".self_attn.out_proj.weight"),
                     P(p + ".self_attn.out_proj.bias"), P(p + ".ffn.linear1.weight"), P(p + ".ffn.linear1.bias"),
                     P(p + ".ffn.linear2.weight"), P(p + ".ffn.linear2.bias"), P(p + ".norm1.weight"),
                     P(p + ".norm1.bias"), P(p + ".norm2.weight"), P(p + ".norm2.bias")};
        L.qkv_p = packed();
        L.out_p = packed();
        L.ff1_p = packed();
        L.ff2_p = packed();
        L.wide_scores = tp.wide_scores[i] != 0;
        ((int)i < cfg->text_encoder_layers ? m->enc : m->dec).push_back(L);
    }
    m->mel_p = packed();
    m->tfused = tp.tfused;
    m->att_f32 = tp.att_f32;
    m->enc_nw = P("text_encoder.norm.weight");
    m->enc_nb = P("text_encoder.norm.bias");
    for (int j = 0; j < 2; ++j) {
        const std::string p = "duration_predictor.predictor.conv_layers." + std::to_string(j) + ".conv.";
        m->dur[4 * j + 0] = m->buf + lay.dw_off + (size_t)j * 3 * H * H;
        m->dur[4 * j + 1] = P(p + "bias");
        m->dur[4 * j + 2] = m->buf + lay.bn_off + (2 * j) * H;
        m->dur[4 * j + 3] = m->buf + lay.bn_off + (2 * j + 1) * H;
    }
    m->dur_split_w[0] = m->buf + lay.dws_off;
    m->dur_split_w[1] = m->buf + lay.dws_off + (size_t)3 * H * H;
    m->dur_split = dp.dur_split;
    m->dur[8] = P("duration_predictor.predictor.projection.weight");
    m->dur[9] = P("duration_predictor.predictor.projection.bias");
    m->dec_nw = P("decoder.norm.weight");
    m->dec_nb = P("decoder.norm.bias");
    m->mel_w = P("decoder.mel_projection.weight");
    m->mel_b = P("decoder.mel_projection.bias");
    // (rw: the same raw vocoder weights as the table of the tails' local redo, below)
    VocRedoW rw;
    rw.M = cfg->mel_channels;
    rw.C = cfg->vocoder_channels;
    m->vin_w = rw.wi = P("vocoder.input_conv.weight");
    m->vin_b = rw.bi = P("vocoder.input_conv.bias");
    for (int k = 0; k < 4; ++k) {
        const std::string u = "vocoder.upsamples." + std::to_string(k);
        const std::string r = "vocoder.resblocks." + std::to_string(k);
        m->up_w[k] = rw.wt[k] = P(u + ".weight");
        m->up_b[k] = rw.bt[k] = P(u + ".bias");
        m->rb_w1[k] = rw.w1[k] = P(r + ".conv1.weight");
        m->rb_b1[k] = rw.b1[k] = P(r + ".conv1.bias");
        m->rb_w2[k] = rw.w2[k] = P(r + ".conv2.weight");
        m->rb_b2[k] = rw.b2[k] = P(r + ".conv2.bias");
    }
    m->vout_w = rw.wo = P("vocoder.output_conv.weight");
    m->vout_b = rw.bo = P("vocoder.output_conv.bias");
    m->fused = vp.fused;
    if (vp.fused) {
        vp.f32.patch(m->vbuf);
        m->vw = vp.vw;
        m->vw.wo = m->vout_w;
        m->vw.bo = m->vout_b;
    }
    if (vp.x3) {
        vp.split.patch(static_cast<uint16_t*>(m->xbuf));
        m->vx = vp.vx;
        m->vx.hcb = reinterpret_cast<const float*>(vp.hcb_at);
        m->vx.hce = reinterpret_cast<const float*>(vp.hce_at);
        m->vx.bi = m->vw.bi;
        for (int k = 0; k < 4; ++k) {
            m->vx.bt[k] = m->vw.bt[k];
            m->vx.b1[k] = m->vw.b1[k];
            m->vx.b2[k] = m->vw.b2[k];
        }
        m->vx.wo = m->vw.wo;
        m->vx.bo = m->vw.bo;
        m->x3 = m->x3_packed = true;
    }
    if ((m->tailp = m->tbuf != nullptr)) {
        const bool s2 = cfg->mel_channels == 80;  // the stage2 tail kernel, else the stage1 one
        (s2 ? m->vx.tp2 : m->vx.tp) = static_cast<const vx_u32x4*>(m->tbuf);
        (s2 ? m->vx.tp2b : m->vx.tpb) =
            reinterpret_cast<const float*>(static_cast<const uint16_t*>(m->tbuf) + vp.tail.bias_at);
    }
    if ((m->midp = m->mbuf != nullptr)) {
        m->vx.mp = static_cast<const vx_u32x4*>(m->mbuf);
        m->vx.mpb = reinterpret_cast<const float*>(static_cast<const uint16_t*>(m->mbuf) + vp.mid.bias_at);
    }

    // ---- auxiliary allocations, then one synchronise: the host vectors above outlive their copies
    const unsigned mapped = hipHostMallocMapped | hipHostMallocCoherent;
    const size_t qbytes = (kTflQueueWords + 16) * sizeof(unsigned);
    void* redo = nullptr;
    g =  // the split path's non-finite-audio flag, host-mapped so the host can read it without a copy
         // (m2_model_check, the M2_E_RANGE check on entry), and the range policy's two device flag words
        ok("hipHostMalloc(range flag)", hipHostMalloc(&m->rflag_host, 64, mapped)) &&
        ok("hipHostGetDevicePointer", hipHostGetDevicePointer(reinterpret_cast<void**>(&m->vx.rflag), m->rflag_host, 0)) &&
        ok("hipMalloc(range flags)", hipMalloc(&m->rflag_dev, 64)) &&
        ok("hipMalloc(range flags)", hipMemsetAsync(m->rflag_dev, 0, 64, st)) &&
        // the local redo's weight table (range policy "fallback" on the pipelined tails, vocoder_redo.h):
        // the raw fp32 vocoder weights (rw), one device copy
        (!(m->tailp || m->fused) || (ok("hipMalloc(redo weights)", hipMalloc(&redo, sizeof(VocRedoW))) &&
                       copy("upload redo weights", redo, &rw, sizeof(VocRedoW), hipMemcpyHostToDevice))) &&
        // work-queue counters of the one-launch transformer layers (TflQueue)
        // (+ 16 words: the count kernel's ticket of the device-T front half)
        ok("hipMalloc(tfl queue)", hipMalloc(&m->tflq, qbytes)) &&
        ok("hipMalloc(tfl queue)", hipMemsetAsync(m->tflq, 0, qbytes, st)) &&
        // the host-mapped [seq, T] pair the back half's first launch posts
        ok("hipHostMalloc(frame post)", hipHostMalloc(&m->fpost_host, 64, mapped | hipHostMallocPortable)) &&
        ok("hipHostGetDevicePointer", hipHostGetDevicePointer(reinterpret_cast<void**>(&m->fpost_dev), m->fpost_host, 0)) &&
        ok("hipStreamSynchronize", hipStreamSynchronize(st));
    m->ragged_w = static_cast<const VocRedoW*>(redo);
    m->redo_w = m->tailp ? m->ragged_w : nullptr;
    if (!g) return failed();
    std::memset(m->rflag_host, 0, 64);
    std::memset(m->fpost_host, 0, 64);
    m->cnt_ticket = m->tflq + kTflQueueWords;
    *out = m;
    return M2_OK;
}

int32_t m2_model_destroy(m2_model* model) {
    if (!model) return M2_OK;
    m2_profile_disable(model);
    if (model->vbuf) (void)hipFree(model->vbuf);
    if (model->xbuf) (void)hipFree(model->xbuf);
    if (model->tbuf) (void)hipFree(model->tbuf);
    if (model->mbuf) (void)hipFree(model->mbuf);
    if (model->rflag_host) (void)hipHostFree(model->rflag_host);
    if (model->rflag_dev) (void)hipFree(model->rflag_dev);
    if (model->tflq) (void)hipFree(model->tflq);
    if (model->fpost_host) (void)hipHostFree(model->fpost_host);
    if (model->ragged_w) (void)hipFree(const_cast<VocRedoW*>(model->ragged_w));
    hipError_t e = hipFree(model->buf);
    delete model;
    if (e != hipSuccess) return hip_status(e, "hipFree(model)");
    return M2_OK;
}

int32_t m2_model_config(const m2_model* model, m2_config* out) {
    M2_CHECK_ARG(model && out, "m2_model_config: null argument");
    *out = model->cfg;
    return M2_OK;
}

}  // extern "C"
