// C-ABI runtime: switch table, stage orchestration (the handle: m2_model.hip).
// See include/m2tts_hip.h for the contract of every entry point.
#include <immintrin.h>

#include <atomic>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "m2_common.h"
#include "m2_model.h"
#include "transformer_fused.h"
#include "transformer_layer.h"
#include "transformer_plan.h"
#include "vocoder_fused.h"

namespace m2 {

namespace {
// The published switch table: an immutable snapshot behind an atomic
// pointer.  reload_switches() (library load, every m2_model_create,
// m2_reload_switches) builds a new one and publishes it only when the
// environment changed; a reader sees one whole snapshot, never a table half
// rewritten by a concurrent creation.  Superseded snapshots are kept (a few
// hundred bytes per environment change), so a reference taken by sw() stays
// valid.  The table is process-wide: creating a handle under a changed
// environment changes the switches of every handle from its next call on.
std::atomic<const Switches*> g_swp{nullptr};
std::mutex g_sw_mu;
int env_int(const char* name, int dflt) {
    const char* e = std::getenv(name);
    return (e && *e) ? std::atoi(e) : dflt;
}
bool env_set(const char* name) { return std::getenv(name) != nullptr; }
bool env_on(const char* name, bool dflt) {  // unset / empty -> dflt, else != "0"
    const char* e = std::getenv(name);
    return (e && *e) ? std::atoi(e) != 0 : dflt;
}
// reloaded when the library loads
const bool g_sw_loaded = (reload_switches(), true);
}  // namespace

const Switches& sw() { return *g_swp.load(std::memory_order_acquire); }

void reload_switches() {
    // zeroed storage, so the padding compares equal between snapshots
    void* raw = std::calloc(1, sizeof(Switches));
    if (!raw) return;  // keep the current table
    Switches& s = *new (raw) Switches();
    const int rb = env_int("M2_DUR_RB", 0);
    s.dur_rb = (rb == 1 || rb == 2) ? rb : 0;
    s.dur_count = std::getenv("M2_DUR_COUNT") && *std::getenv("M2_DUR_COUNT") ? (env_int("M2_DUR_COUNT", 0) != 0) : -1;
    s.speculative = env_on("M2_SPECULATIVE", true) ? 1 : 0;
    s.tf_chain = env_on("M2_TF_CHAIN", true);
    s.tf_layer = env_on("M2_TF_LAYER", true);
    s.tf_unfused = env_set("M2_TF_UNFUSED");
    const int tw = env_int("M2_TF_WAVES", 0);
    s.tf_waves = (tw == 4 || tw == 8) ? tw : 0;
    auto rb124 = [](int v) { return (v == 1 || v == 2 || v == 4) ? v : 0; };
    const int trb = env_int("M2_TFL_RB", 0);
    s.tfl_rb = rb124(trb);
    s.tfl_first_rb = rb124(env_int("M2_TFL_FIRST_RB", 0));
    s.tfl_rb_masked = rb124(env_int("M2_TFL_RB_MASKED", 0));
    s.tfl_rb_unmasked = rb124(env_int("M2_TFL_RB_UNMASKED", 0));
    if (const char* e = std::getenv("M2_TFL_QS2"); e && *e) {
        const int v = std::atoi(e);
        s.tfl_qs2 = (v == 2 || v == 3 || v == 4 || v == 12) ? v : 0;
    }
    s.att_qt = env_int("M2_ATT_QT", 0);
    if (const char* e = std::getenv("M2_ATT_F32")) s.att_f32 = *e && *e != '0';
    s.voc_perlayer = env_set("M2_VOCODER_PERLAYER");
    s.voc_f32 = env_set("M2_VOC_F32");
    s.voc_tail_x3 = env_set("M2_VOC_TAIL_X3");
    s.voc_mid_x3 = env_set("M2_VOC_MID_X3");
    s.voc_plan = env_int("M2_VOC_PLAN", -1);
    s.f32_mt = env_int("M2_F32_MT", 2);
    s.f32_pair = env_int("M2_F32_PAIR", 1) != 0;
    s.f32_comp = env_int("M2_F32_COMP", 1) != 0;
    s.x3_head_prio = env_int("M2_X3_HEAD_PRIO", 0);
    const int mn = env_int("M2_MIDP_NCH", 0);
    s.midp_nch = mn > 0 ? mn : 0;
    const int tn = env_int("M2_TAILP_NCH", 0);
    s.tailp_nch = tn > 0 ? tn : 0;
    s.tailp_seven = env_set("M2_TAILP_SEVEN");
    s.tailp2_nch = env_int("M2_TAILP2_NCH", 0);
    s.tailp2_seven = env_set("M2_TAILP2_SEVEN");
    s.head_inconv = env_set("M2_HEAD_INCONV");
    // "0" or "1"; anything else keeps the default (m2amd.runtime.headmid_switch rejects it at handle creation)
    if (const char* e = std::getenv("M2_HEADMID"); e && (e[0] == '0' || e[0] == '1') && !e[1]) s.headmid = e[0] == '1';
    s.head_items = env_int("M2_HEAD_ITEMS", 1) != 0;
    const int malt = env_int("M2_S2_MID_ALT", -1);
    s.s2_mid_alt = (malt == 0 || malt == 1) ? malt : -1;
    const int htf = env_int("M2_S2_HEAD_TF", env_set("M2_S2_HEAD_TF16") ? 16 : 0);
    s.s2_head_tf = (htf == 16 || htf == 19 || htf == 24 || htf == 27) ? htf : 0;
    s.redo_grid = env_int("M2_REDO_GRID", -1);
    s.redo_launch = env_set("M2_REDO_LAUNCH");
    s.dur_split = env_on("M2_DUR_SPLIT", true);
    s.dur_pers = env_on("M2_DUR_PERS", true);
    std::lock_guard<std::mutex> lk(g_sw_mu);
    const Switches* cur = g_swp.load(std::memory_order_relaxed);
    if (cur && std::memcmp(cur, &s, sizeof(Switches)) == 0) {
        std::free(raw);  // unchanged
        return;
    }
    g_swp.store(&s, std::memory_order_release);  // (never freed: see g_swp)
}

// ---- launchers defined in the kernel translation units ---------------------
int32_t launch_embed_pe(const int64_t*, const float*, const float*, int, int, int, int, float*, const int64_t*,
                        uint8_t*, hipStream_t);
int32_t launch_layer_norm(const float*, const float*, const float*, int, int, float*, hipStream_t);
int32_t launch_linear(const float*, const float*, const float*, const float*, const float*,
                      const float*, int, int, int, int, float*, hipStream_t);
// force_f32: the exact-f32 MFMA attention (a model whose q/k/v bound is outside the split-f16 range)
int32_t launch_attention(const float*, const uint8_t*, int, int, int, int, float*, hipStream_t, bool force_f32 = false);
int32_t launch_duration(const float*, int, int, int, const float* const*, float*, hipStream_t,
                        const float* ln_g = nullptr, const float* ln_b = nullptr, float* enc_out = nullptr,
                        const float* const* wsplit = nullptr);
int32_t launch_duration_count(const float*, int, int, int, const float* const*, float*, hipStream_t, const float*,
                              const float*, float*, float, int32_t*, int32_t*, int32_t*, unsigned*, int32_t*, int32_t,
                              const float* const* wsplit = nullptr);
bool duration_count_fusable(int, int);
int32_t launch_lr_count(const void*, int, float, int, int, int32_t*, int32_t*, int32_t*, hipStream_t);
int32_t launch_lr_count_sync(const void*, int, float, int, int, int32_t*, int32_t*, int32_t*, unsigned*, int32_t*,
                             int32_t, hipStream_t);
int32_t launch_lr_expand(const float*, const int32_t*, int, int, int, int, float*, hipStream_t);
int32_t launch_conv(const float*, const float*, const float*, const float*, const float*,
                    const float*, int, int, bool, int, int, int, int, float*, hipStream_t);
int32_t launch_add_pe(const float*, const float*, int, int, int, float*, hipStream_t);
int32_t launch_embed_pe_scaled(const int64_t*, const float*, const float*, int, int, int, int, float, float*, hipStream_t);
int32_t launch_convT(const float*, const float*, const float*, int, int, int, int, int, int,
                     float*, hipStream_t);
int32_t launch_conv_general(const float*, const float*, const float*, const float*, const float*, const float*, int,
                            int, int, int, int, int, int, int, float*, hipStream_t);
// ragged batches (vocoder_ragged.hip)
int32_t launch_ragged_count(const int32_t*, int, int32_t*, hipStream_t);
int32_t launch_ragged_zero(float*, const int32_t*, int, int, int, hipStream_t);
int32_t launch_ragged_tail(const VocRedoW*, int, int, const float*, bool, const int32_t*, int, int, float*, hipStream_t);
int ragged_window_frames();
int32_t launch_ragged_gather(const float*, bool, const int32_t*, int, int, int, float*, hipStream_t);
int32_t launch_ragged_scatter(const float*, const int32_t*, int, int, float*, hipStream_t);

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }

int32_t fail(int32_t code, const char* what) {
    set_error(what);
    return code;
}

int32_t hip_status(hipError_t e, const char* where) {
    set_error(std::string(where) + ": " + hipGetErrorString(e));
    return static_cast<int32_t>(e);
}

// Receptive field of one audio sample in mel frames, per side: input_conv 1,
// ConvT1 ~1 (two taps), then ResBlock/ConvT stages at 4x..64x, 3 frames in
// total (tools/probe/receptive_field.py propagates the index intervals layer
// by layer).  A window widened by this many frames computes every sample of
// its centre exactly as the whole-utterance call does.
static constexpr int kVocHalo = 3;
// Longest regulated utterance the path accepts: 2^24 mel frames (2^30 audio
// samples, 13.5 h at 22.05 kHz); longer totals (a huge duration_scale or
// target durations) are M2_E_SHAPE, not a wrapped or truncated int32.
static constexpr int32_t kMaxFrames = 1 << 24;

}  // namespace m2

using namespace m2;

namespace {

int32_t mask_kernel_launch(const int64_t* lengths, int B, int S, uint8_t* mask, hipStream_t st);

__global__ void padding_mask_kernel(const int64_t* __restrict__ lengths, int B, int S,
                                    uint8_t* __restrict__ mask) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * S) return;
    const int b = i / S, s = i - b * S;
    mask[i] = (int64_t)s < lengths[b] ? 1 : 0;  // components.py:236-240
}

int32_t mask_kernel_launch(const int64_t* lengths, int B, int S, uint8_t* mask, hipStream_t st) {
    if (B * S == 0) return M2_OK;
    hipLaunchKernelGGL(padding_mask_kernel, dim3(cdiv(B * S, 256)), dim3(256), 0, st, lengths, B, S, mask);
    M2_LAUNCHED("padding_mask_kernel");
    return M2_OK;
}

// Transformer stack scratch: the residual stream x and the padding mask, then
// one region used either by the three-launch layers (qkv, att, hid) or by the
// one-launch layers (two TflBufs sets, ping-pong between layers).
struct TfBufs {
    float *x, *qkv, *att, *hid;
    uint8_t* mask;
    TflBufs tfl[2];
};

template <typename A>
void carve_tf(A& a, int B, int N, int H, int heads, TfBufs* out) {
    const size_t R = (size_t)B * N;
    float* x = a.template take<float>(R * H);
    uint8_t* mask = a.template take<uint8_t>(R);
    const size_t three = align_up(R * 3 * H * 4, 256) + align_up(R * H * 4, 256) + align_up(R * 2 * H * 4, 256);
    const size_t one = tfl_supported(H, heads) ? 2 * align_up(tfl_bytes(B, N, H, heads), 256) : 0;
    unsigned char* region = a.template take<unsigned char>(std::max(three, one));
    if (!out) return;
    *out = TfBufs{};
    out->x = x;
    out->mask = mask;
    if (!region) return;
    out->qkv = reinterpret_cast<float*>(region);
    out->att = reinterpret_cast<float*>(region + align_up(R * 3 * H * 4, 256));
    out->hid = reinterpret_cast<float*>(region + align_up(R * 3 * H * 4, 256) + align_up(R * H * 4, 256));
    if (one) {
        tfl_carve(region, B, N, H, heads, &out->tfl[0]);
        tfl_carve(region + align_up(tfl_bytes(B, N, H, heads), 256), B, N, H, heads, &out->tfl[1]);
    }
}

size_t vocoder_max_cl(const m2_config& c, int T) {
    size_t best = (size_t)c.vocoder_channels * T;
    size_t ch = c.vocoder_channels, L = T;
    for (int k = 0; k < 4; ++k) {
        ch /= 2;
        L *= kRates[k];
        best = std::max(best, ch * L);
    }
    return best;
}

template <typename A>
void carve_voc(A& a, const m2_config& c, int B, int T, float** bufs) {
    const size_t n = (size_t)B * vocoder_max_cl(c, T);
    for (int i = 0; i < 3; ++i) {
        float* p = a.template take<float>(n);
        if (bufs) bufs[i] = p;
    }
}

// Streamed vocoder scratch: the mel window [B, M, W] (or [B, W, M]), its
// audio [B, 64 W] and the vocoder intermediates of a W-frame call, W = the
// widest window (chunk + 2 halo frames, at most T).
struct ChunkBufs {
    float *mel, *audio, *voc[3];
};

template <typename A>
void carve_chunked(A& a, const m2_config& c, int B, int T, int chunk, ChunkBufs* out) {
    const int W = std::min(T, chunk + 2 * kVocHalo);
    float* mel = a.template take<float>((size_t)B * c.mel_channels * W);
    float* audio = a.template take<float>((size_t)B * 64 * W);
    float* voc[3];
    carve_voc(a, c, B, W, voc);
    if (out) *out = ChunkBufs{mel, audio, {voc[0], voc[1], voc[2]}};
}

// Vocoder scratch of a T-frame call on this model (streamed when chunking is
// set and T exceeds one chunk).
size_t vocoder_ws_bytes(const m2_model* m, int B, int T) {
    Sizer s;
    if (m->chunk_frames > 0 && T > m->chunk_frames) carve_chunked(s, m->cfg, B, T, m->chunk_frames, nullptr);
    else carve_voc(s, m->cfg, B, T, nullptr);
    return s.off;
}

// Stage hand-off of m2_inference_front -> m2_inference_back: the encoder
// output, durations, frame prefix sums / totals / maximum and the padding mask.
struct FrontBufs {
    float *enc, *dur;
    int32_t *cum, *tot, *tmax;
    uint8_t* mask;
};

template <typename A>
void carve_front(A& a, int B, int S, int H, FrontBufs* out) {
    float* enc = a.template take<float>((size_t)B * S * H);
    float* dur = a.template take<float>((size_t)B * S);
    int32_t* cum = a.template take<int32_t>((size_t)B * (S + 1));
    int32_t* tot = a.template take<int32_t>((size_t)B);
    int32_t* tmax = a.template take<int32_t>(1);
    uint8_t* mask = a.template take<uint8_t>((size_t)B * S);
    if (out) *out = FrontBufs{enc, dur, cum, tot, tmax, mask};
}

// The next launch's work queue (its parity alternates the counter sets).
TflQueue tfl_queue(const m2_model* m) { return TflQueue{m->tflq, m->tfl_seq++}; }
// A launch that failed may not have zeroed the next counter set: restart both.
int32_t tfl_reset(const m2_model* m, hipStream_t st, int32_t rc) {
    (void)hipMemsetAsync(m->tflq, 0, kTflQueueWords * sizeof(unsigned), st);
    m->tfl_seq = 0;
    return rc;
}

// What plan_transformer (transformer_plan.h) reads of a call on one of this
// model's stacks.
TfCall tf_call(const m2_model* m, bool decoder, TfSrc src, bool masked, bool device_T, bool ragged, int B, int N) {
    const std::vector<m2_layer_w>& layers = decoder ? m->dec : m->enc;
    TfCall c;
    c.decoder = decoder;
    c.H = m->cfg.hidden_dim;
    c.heads = m->cfg.num_heads;
    c.layers = (int)layers.size();
    c.proj = decoder ? m->cfg.mel_channels : 0;
    c.tfused = m->tfused;
    c.att_f32 = m->att_f32;
    for (int l = 0; l < c.layers; ++l)
        if (layers[l].wide_scores) c.set_wide(l);
    c.src = src;
    c.masked = masked;
    c.device_T = device_T;
    c.ragged = ragged;
    c.B = B;
    c.N = N;
    return c;
}

// The pointers of one stack call.  x0: layer 0's input rows [B, N, H] - given
// (src x), or built there by the first launch from ids (embed) or from
// enc / cum / S (expand); x: the stream the layers write (may be x0); out: the
// final projection's output (decoder).
struct TfIo {
    const int64_t* ids = nullptr;
    const float* enc = nullptr;
    const int32_t* cum = nullptr;
    int S = 0;
    float* x0 = nullptr;
    const int64_t* lengths = nullptr;  // masked calls
    uint8_t* mask = nullptr;           // the padding mask the embedding launch writes and the attention reads
    uint8_t* mask_out = nullptr;       // one-launch layers: the caller's mask (may be null), written by tfl_first
    const int32_t* dT = nullptr;       // device frame count: N is the capacity
    const int32_t* rows = nullptr;     // per-utterance rows, N their stride
    float* x = nullptr;
    float* out = nullptr;
};

// Launches the rows of a plan, in order.  Pre-LN layers (components.py:131-140):
// the first layer's residual source is x0, every later launch reads x.
int32_t run_tf_plan(const m2_model* m, const TfPlan& p, const TfIo& io, TfBufs& wb, hipStream_t st) {
    if (p.error.code) return fail(p.error.code, p.error.text);
    const TfCall& c = p.call;
    const std::vector<m2_layer_w>& layers = c.decoder ? m->dec : m->enc;
    const int B = c.B, N = c.N, H = c.H, heads = c.heads, R = B * N, M = c.proj;
    const float* cur = io.x0;
    for (const TfRow& r : p.rows) {
        const m2_layer_w* L = r.layer < c.layers ? &layers[r.layer] : nullptr;
        // what a chained launch runs on its row tile after the layer: the next
        // layer's LN1 -> QKV (next 1) or the final LN -> projection (next 2)
        const m2_layer_w* Nx = r.next == 1 ? &layers[r.layer + 1] : nullptr;
        const float* gn = Nx ? Nx->n1_w : r.next == 2 ? m->dec_nw : nullptr;
        const float* bn = Nx ? Nx->n1_b : r.next == 2 ? m->dec_nb : nullptr;
        const float* Wn = Nx ? Nx->qkv_p : r.next == 2 ? m->mel_p : nullptr;
        const float* bn2 = r.next == 2 ? m->mel_b : nullptr;
        int32_t rc = M2_OK;
        switch (r.kind) {
            case TfKind::EmbedPe:
                rc = launch_embed_pe(io.ids, m->emb, m->pe, B, N, H, m->cfg.vocab_size, io.x0, io.lengths, io.mask, st);
                break;
            case TfKind::EmbedLnGemm:
                rc = launch_embed_ln_gemm(io.ids, m->emb, m->pe, B, N, H, m->cfg.vocab_size, io.lengths, io.mask, io.x0,
                                          L->n1_w, L->n1_b, L->qkv_p, 3 * H, r.waves, wb.qkv, st);
                break;
            case TfKind::LrExpand: rc = launch_lr_expand(io.enc, io.cum, B, io.S, H, N, io.x0, st); break;
            case TfKind::ExpandLnGemm:
                rc = launch_expand_ln_gemm(io.enc, io.cum, B, io.S, N, H, io.x0, L->n1_w, L->n1_b, L->qkv_p, 3 * H,
                                           r.waves, wb.qkv, st);
                break;
            case TfKind::LnGemm:
                rc = launch_ln_gemm(cur, L->n1_w, L->n1_b, L->qkv_p, nullptr, ACT_NONE, R, H, 3 * H, r.waves, wb.qkv, st);
                break;
            case TfKind::Linear:
                if (r.op == 0)
                    rc = launch_linear(cur, L->n1_w, L->n1_b, L->qkv_w, nullptr, nullptr, ACT_NONE, R, H, 3 * H, wb.qkv, st);
                else if (r.op == 1)
                    rc = launch_linear(wb.att, nullptr, nullptr, L->out_w, L->out_b, cur, ACT_NONE, R, H, H, io.x, st);
                else if (r.op == 2)
                    rc = launch_linear(io.x, L->n2_w, L->n2_b, L->ff1_w, L->ff1_b, nullptr, ACT_RELU, R, H, 2 * H, wb.hid, st);
                else
                    rc = launch_linear(wb.hid, nullptr, nullptr, L->ff2_w, L->ff2_b, io.x, ACT_NONE, R, 2 * H, H, io.x, st);
                if (r.op > 0) cur = io.x;
                break;
            case TfKind::Attention:
                rc = launch_attention(wb.qkv, io.mask, B, N, H, heads, wb.att, st, m->att_f32);
                break;
            case TfKind::PostAttn:
                rc = launch_post_attn(wb.att, cur, L->out_p, L->out_b, L->n2_w, L->n2_b, L->ff1_p, L->ff1_b, L->ff2_p,
                                      L->ff2_b, R, H, r.waves, io.x, st);
                cur = io.x;
                break;
            case TfKind::PostAttnNext:
                rc = launch_post_attn_next(wb.att, cur, L->out_p, L->out_b, L->n2_w, L->n2_b, L->ff1_p, L->ff1_b,
                                           L->ff2_p, L->ff2_b, R, H, r.waves, io.x, gn, bn, Wn, bn2,
                                           Nx ? 3 * H : M, Nx ? wb.qkv : io.out, st);
                cur = io.x;
                break;
            case TfKind::TflFirst: {
                TflFirst f;
                f.src = (int)c.src;
                if (c.src == TfSrc::Embed) {
                    f.ids = io.ids;
                    f.emb = m->emb;
                    f.pe = m->pe;
                    f.vocab = m->cfg.vocab_size;
                    f.escale = (float)std::sqrt((double)H);  // as launch_embed_pe
                    f.lengths = io.lengths;
                    f.mask = io.mask_out;
                } else if (c.src == TfSrc::Expand) {  // the length regulator's expansion, built into x0
                    f.enc = io.enc;
                    f.cum = io.cum;
                    f.S = io.S;
                } else {
                    f.x_in = io.x0;
                }
                f.dN = io.dT;
                if (io.dT) {  // the first launch posts T for the host (m2_frames_wait)
                    m->fpost_seq = m->fpost_seq == INT_MAX ? 1 : m->fpost_seq + 1;
                    f.post = m->fpost_dev;
                    f.post_seq = m->fpost_seq;
                }
                rc = launch_tfl_first(f, B, N, H, heads, c.masked, r.rb, io.x0, L->n1_w, L->n1_b, L->qkv_p, wb.tfl[0],
                                      tfl_queue(m), st, io.rows);
                if (rc) return tfl_reset(m, st, rc);
                break;
            }
            case TfKind::TflLayer: {
                TflLayer w{L->out_p, L->out_b, L->n2_w, L->n2_b, L->ff1_p, L->ff1_b, L->ff2_p, L->ff2_b, gn, bn, Wn, bn2};
                rc = launch_tfl_layer(w, B, N, H, heads, c.masked, r.rb, r.qs2, io.lengths, cur, io.x,
                                      wb.tfl[r.layer & 1], r.next, wb.tfl[(r.layer + 1) & 1], r.next == 2 ? M : 0,
                                      r.next == 2 ? io.out : nullptr, tfl_queue(m), st, io.dT, io.rows);
                if (rc) return tfl_reset(m, st, rc);
                cur = io.x;
                break;
            }
            // The decoder's final LayerNorm -> mel projection as a launch of its
            // own (no layer ran it): ln_gemm on the packed weights where (H, mel)
            // has an instance, else - any other mel width of a fused handle, and
            // the fp32 path - the generic linear on the fp32 weights.
            case TfKind::FinalLnGemm:
                rc = launch_ln_gemm(cur, m->dec_nw, m->dec_nb, m->mel_p, m->mel_b, ACT_NONE, R, H, M, r.waves, io.out, st);
                break;
            case TfKind::FinalLinear:
                rc = launch_linear(cur, m->dec_nw, m->dec_nb, m->mel_w, m->mel_b, nullptr, ACT_NONE, R, H, M, io.out, st);
                break;
        }
        if (rc) return rc;
    }
    return M2_OK;
}

}  // namespace

extern "C" {

int32_t m2_abi_version(void) { return M2_ABI_VERSION; }

const char* m2_last_error(void) { return g_last_error.c_str(); }

void m2_reload_switches(void) { reload_switches(); }

size_t m2_workspace_bytes(const m2_model* model, int32_t B, int32_t S, int32_t T) {
    if (!model || B < 0 || S < 0 || T < 0) return 0;
    const int H = model->cfg.hidden_dim;
    Sizer a, b;
    carve_tf(a, B, S, H, model->cfg.num_heads, nullptr);
    carve_tf(b, B, T, H, model->cfg.num_heads, nullptr);
    return std::max(a.off, std::max(b.off, vocoder_ws_bytes(model, B, T))) + 256;
}

}  // extern "C"

namespace {
// TextEncoder.forward up to (not including) the final LayerNorm; *x_pre = the
// last layer's output in the workspace.
int32_t text_encoder_layers(const m2_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t S,
                            uint8_t* out_mask, void* workspace, size_t workspace_bytes, hipStream_t st,
                            float** x_pre) {
    Carve a(workspace, workspace_bytes);
    TfBufs wb;
    carve_tf(a, B, S, m->cfg.hidden_dim, m->cfg.num_heads, &wb);
    if (!a.ok) return fail(M2_E_WORKSPACE, "m2_text_encoder: workspace too small");
    *x_pre = wb.x;
    TfIo io;
    io.ids = ids;
    io.lengths = lengths;
    if (lengths) io.mask = out_mask ? out_mask : wb.mask;  // written by the embedding launch
    io.mask_out = out_mask;
    io.x0 = io.x = wb.x;
    const TfPlan p = plan_transformer(tf_call(m, false, TfSrc::Embed, lengths != nullptr, false, false, B, S), sw());
    return run_tf_plan(m, p, io, wb, st);
}
}  // namespace

extern "C" {

int32_t m2_text_encoder(const m2_model* m, const int64_t* ids, const int64_t* lengths, int32_t B,
                        int32_t S, float* out_enc, uint8_t* out_mask, void* workspace,
                        size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(m && ids && out_enc && B >= 0 && S >= 0, "m2_text_encoder: bad argument");
    M2_CHECK_SHAPE(S <= m->cfg.max_positions, "m2_text_encoder: sequence longer than the positional table");
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* x = nullptr;
    int32_t rc = text_encoder_layers(m, ids, lengths, B, S, out_mask, workspace, workspace_bytes, st, &x);
    if (rc || B == 0 || S == 0) return rc;
    return launch_layer_norm(x, m->enc_nw, m->enc_nb, B * S, m->cfg.hidden_dim, out_enc, st);
}

int32_t m2_duration_predictor(const m2_model* m, const float* enc, int32_t B, int32_t S,
                              float* out_dur, void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace;
    (void)workspace_bytes;
    M2_CHECK_ARG(m && enc && out_dur && B >= 0 && S >= 0, "m2_duration_predictor: bad argument");
    return launch_duration(enc, B, S, m->cfg.hidden_dim, m->dur, out_dur, static_cast<hipStream_t>(stream));
}

int32_t m2_length_regulator_count(const void* dur, int32_t dur_is_int, float scale, int32_t B,
                                  int32_t S, int32_t* out_cum, int32_t* out_T, int32_t* out_Tmax,
                                  void* stream) {
    M2_CHECK_ARG(dur && out_cum && out_T && out_Tmax && B >= 0 && S >= 0, "m2_length_regulator_count: bad argument");
    return launch_lr_count(dur, dur_is_int, scale, B, S, out_cum, out_T, out_Tmax, static_cast<hipStream_t>(stream));
}

// Per-device mailbox of m2_length_regulator_count_sync: [seq, Tmax] in
// coherent host-mapped memory plus the count kernel's ticket counter.
namespace {
struct LrMailbox {
    int32_t* host = nullptr;
    int32_t* dev = nullptr;
    unsigned* ticket = nullptr;
    int32_t seq = 0;
};
constexpr int kMaxDevices = 64;
std::mutex g_mb_mu;
LrMailbox g_mb[kMaxDevices];

// The mailbox's device ticket is zeroed on the caller's stream `st` (and
// waited for): a blocking hipMemset would go to the null stream, which a
// non-blocking stream (e.g. a torch side stream) does not wait for, so the
// first count kernel could take its ticket before the zero landed and never
// post (seen as "stream idle but T_max not posted" on a first call from a
// side stream).
int32_t mailbox_for(int dev, hipStream_t st, LrMailbox** out) {
    LrMailbox& mb = g_mb[dev];
    if (!mb.host) {
        int cur = 0;
        M2_HIP(hipGetDevice(&cur));
        M2_HIP(hipSetDevice(dev));
        void* h = nullptr;
        hipError_t e = hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable);
        void* d = nullptr;
        if (e == hipSuccess) e = hipHostGetDevicePointer(&d, h, 0);
        void* t = nullptr;
        if (e == hipSuccess) e = hipMalloc(&t, sizeof(unsigned));
        (void)hipSetDevice(cur);
        if (e == hipSuccess) e = hipMemsetAsync(t, 0, sizeof(unsigned), st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hip_status(e, "m2_length_regulator_count_sync: mailbox allocation");
        std::memset(h, 0, 64);
        mb.host = static_cast<int32_t*>(h);
        mb.dev = static_cast<int32_t*>(d);
        mb.ticket = static_cast<unsigned*>(t);
    }
    *out = &mb;
    return M2_OK;
}

// Spin on the mailbox until `seq` is posted; every 1024 polls ask the stream
// whether it failed (or finished without posting, which would be a bug).
int32_t mailbox_wait(const LrMailbox* mb, int32_t seq, hipStream_t st, int32_t* host_Tmax, const char* what) {
    for (unsigned i = 1;; ++i) {
        if (__atomic_load_n(mb->host, __ATOMIC_ACQUIRE) == seq) break;
        if ((i & 1023) == 0) {
            const hipError_t e = hipStreamQuery(st);
            if (e == hipSuccess) {
                if (__atomic_load_n(mb->host, __ATOMIC_ACQUIRE) == seq) break;
                return fail(M2_E_INTERNAL, (std::string(what) + ": stream idle but T_max not posted").c_str());
            }
            if (e != hipErrorNotReady) return hip_status(e, what);
        }
        _mm_pause();
    }
    *host_Tmax = __atomic_load_n(mb->host + 1, __ATOMIC_RELAXED);
    return M2_OK;
}

int32_t stream_device(hipStream_t st, int* dev) {
    if (st) M2_HIP(hipStreamGetDevice(st, dev));
    else M2_HIP(hipGetDevice(dev));
    M2_CHECK_ARG(*dev >= 0 && *dev < kMaxDevices, "T_max mailbox: device index");
    return M2_OK;
}
}  // namespace

int32_t m2_length_regulator_count_sync(const void* dur, int32_t dur_is_int, float scale, int32_t B, int32_t S,
                                       int32_t* out_cum, int32_t* out_T, int32_t* out_Tmax, int32_t* host_Tmax,
                                       void* stream) {
    M2_CHECK_ARG(out_Tmax && host_Tmax && B >= 0 && S >= 0, "m2_length_regulator_count_sync: bad argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (B == 0) {  // empty batch: the [0, ...] tensors have no storage
        M2_HIP(hipMemsetAsync(out_Tmax, 0, sizeof(int32_t), st));
        *host_Tmax = 0;
        return M2_OK;
    }
    M2_CHECK_ARG(dur && out_cum && out_T, "m2_length_regulator_count_sync: bad argument");
    int dev = 0;
    int32_t rc0 = stream_device(st, &dev);
    if (rc0) return rc0;
    std::lock_guard<std::mutex> lk(g_mb_mu);
    LrMailbox* mb = nullptr;
    int32_t rc = mailbox_for(dev, st, &mb);
    if (rc) return rc;
    mb->seq = mb->seq == INT_MAX ? 1 : mb->seq + 1;
    const int32_t seq = mb->seq;
    if ((rc = launch_lr_count_sync(dur, dur_is_int, scale, B, S, out_cum, out_T, out_Tmax, mb->ticket, mb->dev, seq,
                                   st)))
        return rc;
    if ((rc = mailbox_wait(mb, seq, st, host_Tmax, "m2_length_regulator_count_sync"))) return rc;
    M2_CHECK_SHAPE(*host_Tmax <= kMaxFrames, "length regulator: an utterance's frame count exceeds 2^24 (the "
                                             "durations times duration_scale are out of range)");
    return M2_OK;
}

int32_t m2_length_regulator_expand(const float* enc, const int32_t* cum, int32_t B, int32_t S,
                                   int32_t H, int32_t T_out, float* out, void* stream) {
    M2_CHECK_ARG(enc && cum && out && B >= 0 && S >= 0 && H > 0 && T_out >= 0, "m2_length_regulator_expand: bad argument");
    return launch_lr_expand(enc, cum, B, S, H, T_out, out, static_cast<hipStream_t>(stream));
}

}  // extern "C"

namespace {
// The mel decoder on x [B, T, H]; with enc / cum given, x is first filled by
// the length regulator's frame expansion of enc (by the first layer's launch
// where the plan fuses it, else a separate lr_expand launch).
// dT: T is the capacity of a speculative launch, the frame count a device word.
// rows (one-launch layers only): utterance b has rows[b] frames, T is the
// row stride; out_mel's rows past rows[b] are then not written.
int32_t mel_decoder(const m2_model* m, float* x, int32_t B, int32_t T, float* out_mel, void* workspace,
                    size_t workspace_bytes, hipStream_t st, const float* enc = nullptr, const int32_t* cum = nullptr,
                    int32_t S = 0, const int32_t* dT = nullptr, const int32_t* rows = nullptr) {
    Carve a(workspace, workspace_bytes);
    TfBufs wb;
    carve_tf(a, B, T, m->cfg.hidden_dim, m->cfg.num_heads, &wb);
    if (!a.ok) return fail(M2_E_WORKSPACE, "m2_mel_decoder: workspace too small");
    TfIo io;
    io.enc = enc;
    io.cum = cum;
    io.S = S;
    io.x0 = x;
    io.dT = dT;
    io.rows = rows;
    io.x = wb.x;
    io.out = out_mel;
    const TfPlan p = plan_transformer(
        tf_call(m, true, enc ? TfSrc::Expand : TfSrc::X, false, dT != nullptr, rows != nullptr, B, T), sw());
    return run_tf_plan(m, p, io, wb, st);
}
}  // namespace

extern "C" {

int32_t m2_mel_decoder(const m2_model* m, const float* x, int32_t B, int32_t T, float* out_mel,
                       void* workspace, size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(m && x && out_mel && B >= 0 && T >= 0, "m2_mel_decoder: bad argument");
    return mel_decoder(m, const_cast<float*>(x), B, T, out_mel, workspace, workspace_bytes,
                       static_cast<hipStream_t>(stream));
}

}  // extern "C"

namespace {
int32_t vocoder_run(const m2_model* m, const float* mel, int32_t mel_layout, int32_t B, int32_t T, float* out_audio,
                    float* const* buf, hipStream_t st, bool x3, int redo = -1, const int32_t* dT = nullptr);

// Audio samples [64 f0, 64 f1) of every utterance of a T-frame mel, computed
// over the window [f0 - halo, f1 + halo) clipped to [0, T): the window's mel
// rows are copied to c.mel (same layout, T_w frames), vocoded as a T_w-frame
// call, and the centre of its audio copied to out (row pitch out_pitch floats,
// utterance b's chunk at out + b * out_pitch).
int32_t vocoder_window(const m2_model* m, const float* mel, int32_t layout, int32_t B, int32_t T, int32_t f0,
                       int32_t f1, float* out, size_t out_pitch, const ChunkBufs& c, hipStream_t st, bool x3,
                       int redo = -1) {
    const int M = m->cfg.mel_channels;
    const int w0 = std::max(0, f0 - kVocHalo), w1 = std::min(T, f1 + kVocHalo), W = w1 - w0;
    if (layout == 1)  // [B,T,M]: utterance b's window is W*M contiguous floats
        M2_HIP(hipMemcpy2DAsync(c.mel, (size_t)W * M * 4, mel + (size_t)w0 * M, (size_t)T * M * 4, (size_t)W * M * 4, B,
                                hipMemcpyDeviceToDevice, st));
    else  // [B,M,T]: one W-float row per (utterance, channel)
        M2_HIP(hipMemcpy2DAsync(c.mel, (size_t)W * 4, mel + w0, (size_t)T * 4, (size_t)W * 4, (size_t)B * M,
                                hipMemcpyDeviceToDevice, st));
    int32_t rc = vocoder_run(m, c.mel, layout, B, W, c.audio, c.voc, st, x3, redo);
    if (rc) return rc;
    M2_HIP(hipMemcpy2DAsync(out, out_pitch * 4, c.audio + (size_t)64 * (f0 - w0), (size_t)64 * W * 4,
                            (size_t)64 * (f1 - f0) * 4, B, hipMemcpyDeviceToDevice, st));
    return M2_OK;
}

// One m2_vocoder call on the split (x3) or exact-f32 kernels; redo >= 0: the
// on-device range redo with flag word redo (vocoder_run).
int32_t vocoder_call(const m2_model* m, const float* mel, int32_t mel_layout, int32_t B, int32_t T, float* out_audio,
                     void* workspace, size_t workspace_bytes, hipStream_t st, bool x3, int redo = -1,
                     const int32_t* dT = nullptr) {
    Carve a(workspace, workspace_bytes);
    M2_CHECK_ARG(!dT || (m->fused && !(m->chunk_frames > 0 && T > m->chunk_frames)),
                 "m2_vocoder: a device frame count needs the fused, unchunked vocoder");
    if (m->chunk_frames > 0 && T > m->chunk_frames) {  // streamed: chunk by chunk into out_audio
        ChunkBufs c;
        carve_chunked(a, m->cfg, B, T, m->chunk_frames, &c);
        if (!a.ok) return fail(M2_E_WORKSPACE, "m2_vocoder: workspace too small");
        if (B == 0) return M2_OK;
        for (int f0 = 0; f0 < T; f0 += m->chunk_frames) {
            const int f1 = std::min(T, f0 + m->chunk_frames);
            const int32_t rc = vocoder_window(m, mel, mel_layout, B, T, f0, f1, out_audio + (size_t)64 * f0,
                                              (size_t)64 * T, c, st, x3, redo);
            if (rc) return rc;
        }
        return M2_OK;
    }
    float* buf[3];
    carve_voc(a, m->cfg, B, T, buf);
    if (!a.ok) return fail(M2_E_WORKSPACE, "m2_vocoder: workspace too small");
    if (B == 0 || T == 0) return M2_OK;
    return vocoder_run(m, mel, mel_layout, B, T, out_audio, buf, st, x3, redo, dT);
}

// Sticky range error of an earlier call (policy 0), returned and cleared on entry.
int32_t range_entry(const m2_model* m, const char* what) {
    if (m->rflag_host && __atomic_load_n(m->rflag_host, __ATOMIC_ACQUIRE)) {
        __atomic_store_n(m->rflag_host, 0, __ATOMIC_RELEASE);
        return fail(M2_E_RANGE, (std::string(what) + ": an earlier vocoder call on this model produced non-finite "
                                 "audio on the split-f16 path (an input or activation of magnitude >= 65520, or "
                                 "a non-finite input); its output is invalid - re-run it with "
                                 "m2_vocoder_select(model, 1) or range policy 1").c_str());
    }
    return M2_OK;
}

// Policy 1 on the fused vocoders: the flag word of this call for an on-device
// redo (vocoder_run), or -1 (the host-side fallback below).
int device_redo_word(const m2_model* m, bool x3) {
    if (m->range_policy != 1 || !x3 || !m->fused || !m->rflag_dev) return -1;
    return (int)(m->rseq++ & 1u);
}

// Policy 1 otherwise: wait for the call, and re-run it on the exact-f32
// kernels if its audio came out non-finite.
template <typename F>
int32_t range_fallback(const m2_model* m, hipStream_t st, bool x3, F redo) {
    if (m->range_policy != 1 || !x3 || !m->rflag_host) return M2_OK;
    M2_HIP(hipStreamSynchronize(st));
    if (!__atomic_load_n(m->rflag_host, __ATOMIC_ACQUIRE)) return M2_OK;
    __atomic_store_n(m->rflag_host, 0, __ATOMIC_RELEASE);
    return redo();
}

// m2_vocoder; dT: T is the capacity of a speculative launch (dev_frames)
int32_t vocoder_entry(const m2_model* m, const float* mel, int32_t mel_layout, int32_t B, int32_t T, float* out_audio,
                      void* workspace, size_t workspace_bytes, void* stream, const int32_t* dT = nullptr) {
    M2_CHECK_ARG(m && mel && out_audio && B >= 0 && T >= 0, "m2_vocoder: bad argument");
    M2_CHECK_ARG(mel_layout == 0 || mel_layout == 1, "m2_vocoder: mel_layout must be 0 or 1");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t rc = range_entry(m, "m2_vocoder");
    if (rc) return rc;
    const bool x3 = m->x3;
    const int redo = device_redo_word(m, x3);
    if ((rc = vocoder_call(m, mel, mel_layout, B, T, out_audio, workspace, workspace_bytes, st, x3, redo, dT)))
        return rc;
    if (redo >= 0) return M2_OK;
    return range_fallback(m, st, x3, [&] {
        return vocoder_call(m, mel, mel_layout, B, T, out_audio, workspace, workspace_bytes, st, false, -1, dT);
    });
}
}  // namespace

extern "C" {

int32_t m2_vocoder(const m2_model* m, const float* mel, int32_t mel_layout, int32_t B, int32_t T,
                   float* out_audio, void* workspace, size_t workspace_bytes, void* stream) {
    return vocoder_entry(m, mel, mel_layout, B, T, out_audio, workspace, workspace_bytes, stream);
}

int32_t m2_vocoder_chunk(const m2_model* m, const float* mel, int32_t mel_layout, int32_t B, int32_t T, int32_t f0,
                         int32_t f1, float* out_chunk, void* workspace, size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(m && mel && out_chunk && B >= 0 && T >= 0, "m2_vocoder_chunk: bad argument");
    M2_CHECK_ARG(mel_layout == 0 || mel_layout == 1, "m2_vocoder_chunk: mel_layout must be 0 or 1");
    M2_CHECK_ARG(0 <= f0 && f0 < f1 && f1 <= T, "m2_vocoder_chunk: need 0 <= f0 < f1 <= T");
    int32_t rc = range_entry(m, "m2_vocoder_chunk");
    if (rc) return rc;
    Carve a(workspace, workspace_bytes);
    ChunkBufs c;
    carve_chunked(a, m->cfg, B, T, f1 - f0, &c);
    if (!a.ok) return fail(M2_E_WORKSPACE, "m2_vocoder_chunk: workspace too small");
    if (B == 0) return M2_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool x3 = m->x3;
    const int redo = device_redo_word(m, x3);
    if ((rc = vocoder_window(m, mel, mel_layout, B, T, f0, f1, out_chunk, (size_t)64 * (f1 - f0), c, st, x3, redo)))
        return rc;
    if (redo >= 0) return M2_OK;
    return range_fallback(m, st, x3, [&] {
        return vocoder_window(m, mel, mel_layout, B, T, f0, f1, out_chunk, (size_t)64 * (f1 - f0), c, st, false);
    });
}

int32_t m2_set_range_policy(m2_model* m, int32_t policy) {
    M2_CHECK_ARG(m && (policy == 0 || policy == 1), "m2_set_range_policy: policy must be 0 (report) or 1 (fallback)");
    m->range_policy = policy;
    return M2_OK;
}

int32_t m2_model_check(m2_model* m, void* stream, int32_t* flagged) {
    M2_CHECK_ARG(m && flagged, "m2_model_check: bad argument");
    M2_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    *flagged = m->rflag_host ? __atomic_exchange_n(m->rflag_host, 0, __ATOMIC_ACQ_REL) : 0;
    return M2_OK;
}

size_t m2_vocoder_chunk_workspace_bytes(const m2_model* m, int32_t B, int32_t T, int32_t chunk_frames) {
    if (!m || B < 0 || T < 0 || chunk_frames <= 0) return 0;
    Sizer s;
    carve_chunked(s, m->cfg, B, T, chunk_frames, nullptr);
    return s.off + 256;
}

int32_t m2_vocoder_set_chunking(m2_model* m, int32_t chunk_frames) {
    M2_CHECK_ARG(m && chunk_frames >= 0, "m2_vocoder_set_chunking: bad argument");
    m->chunk_frames = chunk_frames;
    return M2_OK;
}

int32_t m2_vocoder_halo_frames(void) { return kVocHalo; }

int32_t m2_vocoder_select(m2_model* m, int32_t path) {
    M2_CHECK_ARG(m, "m2_vocoder_select: null model");
    if (path == 2) {
        M2_CHECK_ARG(m->x3_packed, "m2_vocoder_select: no split-f16 packs (shape unsupported, weights outside the "
                                   "f16 range or M2_VOC_F32 set at creation)");
        m->x3 = true;
        return M2_OK;
    }
    M2_CHECK_ARG(path == 1 && m->fused, "m2_vocoder_select: path must be 1 (exact-f32) or 2 (split-f16)");
    m->x3 = false;
    return M2_OK;
}

}  // extern "C"

namespace {
// What a call is, for the launch plan (vocoder_launch.h).
VocCall voc_call(const m2_model* m, int32_t mel_layout, int32_t B, int32_t T, bool x3, int redo, bool device_T,
                 unsigned prof_slots) {
    VocCall c;
    c.M = m->cfg.mel_channels, c.C = m->cfg.vocoder_channels;
    c.B = B, c.T = T;
    c.trans = mel_layout == 1;
    c.device_T = device_T;
    c.prof_slots = prof_slots;
    c.hc = m->vx.hc, c.mp = m->vx.mp, c.tp = m->vx.tp, c.tp2 = m->vx.tp2, c.redo_w = m->redo_w;
    c.wt4p = m->vw.wt4p, c.hcw = m->vw.hcw;
    c.fused = m->fused, c.x3 = x3;
    c.range_policy = m->range_policy, c.redo = redo;
    return c;
}

// redo >= 0 (range policy 1, x3): the split kernels raise flag word `redo`
// instead of the host-mapped flag, and the exact-f32 kernels follow, each
// workgroup returning at once unless that word is raised - a call whose split
// audio came out non-finite is recomputed on the device, with no host wait.
// The call is planned once (plan_vocoder_launch); the launchers decide nothing.
int32_t vocoder_run(const m2_model* m, const float* mel, int32_t mel_layout, int32_t B, int32_t T, float* out_audio,
                    float* const* buf, hipStream_t st, bool x3, int redo, const int32_t* dT) {
    int32_t rc;
    if (m->fused) {
        const int call = m->prof_calls;
        const bool rec = (size_t)(call + 1) * kVocKernels <= m->prof_begin.size() &&
                         m->prof_seen++ % m->prof_stride == 0;
        if (rec) m->prof_calls++;
        auto mark = [&](int kidx, bool begin) {
            if (!rec || !((m->prof_mask >> kidx) & 1u)) return;
            const size_t slot = (size_t)call * kVocKernels + kidx;
            (void)hipEventRecord(begin ? m->prof_begin[slot] : m->prof_end[slot], st);
        };
        VocX vx = m->vx;
        VocW vw = m->vw;
        vx.dT = vw.dT = dT;
        vx.head_prio = sw().x3_head_prio;
        vx.prof_slots = rec ? m->prof_mask : 0u;
        const VocLaunchPlan plan = plan_vocoder_launch(voc_call(m, mel_layout, B, T, x3, redo, dT != nullptr, vx.prof_slots),
                                                       sw(), x3 ? vocoder_x3_slots() : VocSlots{});
        if (plan.path == VocPath::F32) return launch_vocoder_fused(mel, T, plan, vw, buf[0], buf[1], out_audio, st, mark);
        if (plan.redo == VocRedoPlan::InTail || plan.redo == VocRedoPlan::Guarded) {
            vx.rflag = m->rflag_dev + redo;
            vx.rclear = m->rflag_dev + (redo ^ 1);
            vx.rqueue = reinterpret_cast<unsigned*>(m->rflag_dev + 4);
        }
        if (plan.redo == VocRedoPlan::InTail) vx.redo_w = m->redo_w;  // the tail's local fp32 redo
        if ((rc = launch_vocoder_x3(mel, T, plan, vx, buf[0], buf[1], out_audio, st, mark))) return rc;
        if (plan.redo != VocRedoPlan::Guarded) return M2_OK;
        vw.guard = m->rflag_dev + redo;
        vw.guard_queue = reinterpret_cast<const unsigned*>(m->rflag_dev + 4);  // words 4-7 (zeroed by the head)
        return launch_vocoder_fused(mel, T, plan, vw, buf[0], buf[1], out_audio, st, [](int, bool) {});
    }
    M2_CHECK_ARG(!dT, "m2_vocoder: a device frame count needs the fused vocoder");
    int ch = m->cfg.vocoder_channels, L = T;
    float *cur = buf[0], *up = buf[1], *tmp = buf[2];
    if ((rc = launch_conv(mel, m->vin_w, m->vin_b, nullptr, nullptr, nullptr, 3, ACT_NONE, mel_layout == 1, B, m->cfg.mel_channels, ch, L, cur, st))) return rc;
    for (int k = 0; k < 4; ++k) {
        if ((rc = launch_convT(cur, m->up_w[k], m->up_b[k], kRates[k], ACT_LEAKY, B, ch, ch / 2, L, up, st))) return rc;
        ch /= 2;
        L *= kRates[k];
        if ((rc = launch_conv(up, m->rb_w1[k], m->rb_b1[k], nullptr, nullptr, nullptr, 3, ACT_LEAKY, false, B, ch, ch, L, tmp, st))) return rc;
        if ((rc = launch_conv(tmp, m->rb_w2[k], m->rb_b2[k], nullptr, nullptr, up, 3, ACT_NONE, false, B, ch, ch, L, cur, st))) return rc;
    }
    return launch_conv(cur, m->vout_w, m->vout_b, nullptr, nullptr, nullptr, 3, ACT_TANH, false, B, ch, 1, L, out_audio, st);
}
}  // namespace

extern "C" {

int32_t m2_vocoder_resblock(const m2_model* m, int32_t k, const float* x, int32_t B, int32_t L,
                            float* y, float* tmp, void* stream) {
    M2_CHECK_ARG(m && x && y && tmp && k >= 0 && k < 4 && B >= 0 && L >= 0, "m2_vocoder_resblock: bad argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int ch = m->cfg.vocoder_channels >> (k + 1);
    int32_t rc;
    if ((rc = launch_conv(x, m->rb_w1[k], m->rb_b1[k], nullptr, nullptr, nullptr, 3, ACT_LEAKY, false, B, ch, ch, L, tmp, st))) return rc;
    return launch_conv(tmp, m->rb_w2[k], m->rb_b2[k], nullptr, nullptr, x, 3, ACT_NONE, false, B, ch, ch, L, y, st);
}

int32_t m2_vocoder_upsample(const m2_model* m, int32_t k, const float* x, int32_t B, int32_t L,
                            float* y, void* stream) {
    M2_CHECK_ARG(m && x && y && k >= 0 && k < 4 && B >= 0 && L >= 0, "m2_vocoder_upsample: bad argument");
    const int ch = m->cfg.vocoder_channels >> k;
    return launch_convT(x, m->up_w[k], m->up_b[k], kRates[k], ACT_LEAKY, B, ch, ch / 2, L, y, static_cast<hipStream_t>(stream));
}

int32_t m2_conv1d(const float* x, const float* w, const float* b, const float* alpha,
                  const float* beta, const float* res, int32_t ksize, int32_t act, int32_t B,
                  int32_t Cin, int32_t Cout, int32_t L, float* y, void* stream) {
    M2_CHECK_ARG(x && w && b && y && B >= 0 && L >= 0 && act >= 0 && act <= 4, "m2_conv1d: bad argument");
    return launch_conv(x, w, b, alpha, beta, res, ksize, act, false, B, Cin, Cout, L, y, static_cast<hipStream_t>(stream));
}

int32_t m2_conv1d_ex(const float* x, const float* w, const float* b, const float* alpha, const float* beta,
                     const float* res, int32_t ksize, int32_t dilation, int32_t padding, int32_t act, int32_t B,
                     int32_t Cin, int32_t Cout, int32_t L, float* y, void* stream) {
    M2_CHECK_ARG(x && w && b && y && B >= 0 && L >= 0, "m2_conv1d_ex: bad argument");
    return launch_conv_general(x, w, b, alpha, beta, res, ksize, dilation, padding, act, B, Cin, Cout, L, y,
                               static_cast<hipStream_t>(stream));
}

int32_t m2_conv_transpose1d(const float* x, const float* w, const float* b, int32_t rate,
                            int32_t act, int32_t B, int32_t Cin, int32_t Cout, int32_t L, float* y,
                            void* stream) {
    M2_CHECK_ARG(x && w && b && y && B >= 0 && L >= 0 && act >= 0 && act <= 3, "m2_conv_transpose1d: bad argument");
    return launch_convT(x, w, b, rate, act, B, Cin, Cout, L, y, static_cast<hipStream_t>(stream));
}

int32_t m2_linear(const float* x, const float* gamma, const float* beta, const float* w,
                  const float* b, const float* res, int32_t act, int32_t R, int32_t K, int32_t N,
                  float* y, void* stream) {
    M2_CHECK_ARG(x && w && y && R >= 0 && (act == ACT_NONE || act == ACT_RELU), "m2_linear: bad argument");
    M2_CHECK_ARG((gamma == nullptr) == (beta == nullptr), "m2_linear: gamma and beta go together");
    return launch_linear(x, gamma, beta, w, b, res, act, R, K, N, y, static_cast<hipStream_t>(stream));
}

int32_t m2_layer_norm(const float* x, const float* gamma, const float* beta, int32_t R, int32_t K,
                      float* y, void* stream) {
    M2_CHECK_ARG(x && gamma && beta && y && R >= 0 && K > 0, "m2_layer_norm: bad argument");
    return launch_layer_norm(x, gamma, beta, R, K, y, static_cast<hipStream_t>(stream));
}

int32_t m2_attention(const float* qkv, const uint8_t* key_mask, int32_t B, int32_t N, int32_t H,
                     int32_t heads, float* out, void* stream) {
    M2_CHECK_ARG(qkv && out && B >= 0 && N >= 0 && H > 0 && heads > 0, "m2_attention: bad argument");
    return launch_attention(qkv, key_mask, B, N, H, heads, out, static_cast<hipStream_t>(stream));
}

int32_t m2_embed_positional(const int64_t* ids, const float* emb, const float* pe, int32_t B,
                            int32_t S, int32_t H, int32_t vocab, float scale, float* y,
                            void* stream) {
    M2_CHECK_ARG(ids && emb && pe && y && B >= 0 && S >= 0 && H > 0 && vocab > 0, "m2_embed_positional: bad argument");
    return launch_embed_pe_scaled(ids, emb, pe, B, S, H, vocab, scale, y, static_cast<hipStream_t>(stream));
}

int32_t m2_add_positional(const float* x, const float* pe, int32_t B, int32_t S, int32_t H,
                          float* y, void* stream) {
    M2_CHECK_ARG(x && pe && y && B >= 0 && S >= 0 && H > 0, "m2_add_positional: bad argument");
    return launch_add_pe(x, pe, B, S, H, y, static_cast<hipStream_t>(stream));
}

int32_t m2_profile_kernel_count(void) { return kVocKernels; }

const char* m2_profile_kernel_name(int32_t index) {
    return (index >= 0 && index < kVocKernels) ? kVocKernelNames[index] : "";
}

const char* m2_profile_kernel_name_for(const m2_model* m, int32_t index) {
    if (!m || index < 0 || index >= kVocKernels) return "";
    if (m->x3 && index == 1 && voc_mid_kind(m->vx.mp) == VocMid::Midp) return kVocMidpKernelName;
    if (m->x3 && index == 2) {
        const VocTail t = voc_tail_kind(m->vx.tp, m->vx.tp2);
        if (t != VocTail::X3) return t == VocTail::Tailp2 ? kVocTailp2KernelName : kVocTailpKernelName;
    }
    return m->x3 ? kVocX3KernelNames[index] : kVocKernelNames[index];
}

int32_t m2_debug_vocoder_plan(const m2_model* m, int32_t B, int32_t T, int32_t mel_layout, int32_t device_T, char* out,
                              size_t cap) {
    M2_CHECK_ARG(m && B > 0 && T > 0 && (mel_layout == 0 || mel_layout == 1), "m2_debug_vocoder_plan: bad argument");
    // the flag word an m2_vocoder call would get now (device_redo_word, without advancing it)
    const int redo = m->range_policy == 1 && m->x3 && m->fused && m->rflag_dev ? (int)(m->rseq & 1u) : -1;
    const VocCall c = voc_call(m, mel_layout, B, T, m->x3, redo, device_T != 0, 0u);
    const VocLaunchPlan p = plan_vocoder_launch(c, sw(), m->x3 && m->fused ? vocoder_x3_slots() : VocSlots{});
    return p.print(out, cap);
}

size_t m2_front_bytes(const m2_model* model, int32_t B, int32_t S) {
    if (!model || B < 0 || S < 0) return 0;
    Sizer a;
    carve_front(a, B, S, model->cfg.hidden_dim, nullptr);
    return a.off + 256;
}

}  // extern "C"

namespace {
// The front half up to the frame counts: encoder, durations (into f), then
// the frame counts.  With `fuse` (and a batch small enough, fuse_count) the
// duration kernel's last workgroup runs the count itself: T_max into fuse->Tmax, the ticket
// fuse->ticket, the optional mailbox post; otherwise count(f) launches the
// length regulator's count kernel.
struct CountFuse {
    float scale;
    int32_t* Tmax;  // null: the front buffer's own T_max word
    unsigned* ticket;
    int32_t* mbox;
    int32_t seq;
};
// Default: fused for B * S <= 2048.  The last workgroup's count is serial
// work behind every other workgroup: at stage2 B=8 S=100 the step is 1.9 %
// shorter fused (duration 13.3 -> 15.7 us, the 5 us count launch gone), at
// stage1 B=32 and stage2 B=64 S=100 it measured +0.3 / +0.7 % (in-process
// A/B, profiles/r03/r03aa_ab.txt; again on the round-6 tree, stage1 B=32
// S=100: 0.1455 -> 0.1469 ms fused, profiles/r06/r06z12_count_ab.txt).
// M2_DUR_COUNT=1 fuses up to the kernel's limit (8192), =0 never.
bool fuse_count(int B, int S) {
    if (sw().dur_count >= 0) return sw().dur_count != 0 && duration_count_fusable(B, S);
    return (long)B * S <= 2048 && duration_count_fusable(B, S);
}
template <typename Count>
int32_t front_run(const m2_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t S, void* front,
                  size_t front_bytes, void* workspace, size_t workspace_bytes, hipStream_t st, FrontBufs* f,
                  Count count, const CountFuse* fuse = nullptr) {
    M2_CHECK_ARG(m && B >= 0 && S >= 0, "m2_inference_front: bad argument");
    M2_CHECK_ARG(ids || B * S == 0, "m2_inference_front: null ids");
    if (int32_t rc0 = range_entry(m, "m2_inference")) return rc0;
    Carve a(front, front_bytes);
    carve_front(a, B, S, m->cfg.hidden_dim, f);
    if (!a.ok) return fail(M2_E_WORKSPACE, "m2_inference_front: front buffer too small");
    int32_t rc;
    if (B > 0 && S > 0) {
        M2_CHECK_SHAPE(S <= m->cfg.max_positions, "m2_inference: sequence longer than the positional table");
        float* x = nullptr;
        if ((rc = text_encoder_layers(m, ids, lengths, B, S, lengths ? f->mask : nullptr, workspace, workspace_bytes,
                                      st, &x)))
            return rc;
        // the encoder's final LayerNorm runs inside the duration kernel, which
        // also stores the normalised encoder output (f.enc)
        // (split-f16 convs when the static range bound allows: dur_split)
        const float* const* ws = m->dur_split && sw().dur_split ? m->dur_split_w : nullptr;
        if (fuse && fuse_count(B, S))
            return launch_duration_count(x, B, S, m->cfg.hidden_dim, m->dur, f->dur, st, m->enc_nw, m->enc_nb, f->enc,
                                         fuse->scale, f->cum, f->tot, fuse->Tmax ? fuse->Tmax : f->tmax,
                                         fuse->ticket, fuse->mbox, fuse->seq, ws);
        if ((rc = launch_duration(x, B, S, m->cfg.hidden_dim, m->dur, f->dur, st, m->enc_nw, m->enc_nb, f->enc, ws)))
            return rc;
    }
    // Round 1's fused count (per-utterance tickets behind release fences: one
    // L2 write-back per workgroup) measured 5 us slower than this separate
    // kernel (tools/probe/count_fusion_ab.py, r17); the fused form above hands
    // the durations over with write-through stores instead.
    return count(*f);
}

// Ragged batches need the kernels that take a per-utterance bound: the
// one-launch layers (decoder) and the fused vocoder with its fp32 weight table
// for the end fix-up (vocoder).  Otherwise M2_E_SHAPE: the caller runs the
// utterances one by one.
int32_t ragged_supported(const m2_model* m, bool decoder, bool vocoder, const char* what) {
    if (decoder) {  // the refusal a ragged decoder call would plan to, under the entry point's name
        const TfError e = tf_call_error(tf_call(m, true, TfSrc::X, false, false, true, 1, 1), sw());
        if (e.code) return fail(e.code, (std::string(what) + ": " + e.text).c_str());
    }
    if (vocoder && !(m->fused && m->ragged_w))
        return fail(M2_E_SHAPE, (std::string(what) + ": per-utterance frame counts need the fused vocoder "
                                 "(unsupported (mel_channels, vocoder_channels) or M2_VOCODER_PERLAYER)").c_str());
    return M2_OK;
}

// Scratch of the end-window pass for B utterances (the mel windows, their
// audio, the vocoder intermediates of a window-long call): what the ragged
// vocoder needs beside the plain call's workspace (m2_ragged_workspace_bytes).
size_t ragged_extra_bytes(const m2_model* m, int B) {
    const int W = ragged_window_frames();
    Sizer s;
    carve_chunked(s, m->cfg, B, W, W, nullptr);
    return s.off + 256;
}

// The batched vocoder at T frames, then each utterance's end redone at its own
// length frames[b] and everything past it cleared (vocoder_ragged.hip): one
// more call of the selected vocoder kernels on the utterances' end windows,
// the fp32 kernel for utterances shorter than a window.  The main pass may be
// split-f16, exact-f32 or streamed: the fix-up only replaces its audio.
// win: ragged_extra_bytes(m, B) of scratch for the window pass.
int32_t vocoder_ragged(const m2_model* m, const float* mel, int32_t mel_layout, const int32_t* frames, int32_t B,
                       int32_t T, float* out_audio, void* workspace, size_t workspace_bytes, void* win, size_t win_bytes,
                       void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t rc = vocoder_entry(m, mel, mel_layout, B, T, out_audio, workspace, workspace_bytes, stream);
    if (rc || B == 0 || T == 0) return rc;
    const int W = ragged_window_frames(), M = m->cfg.mel_channels;
    if (T > W) {  // else no utterance is both shorter than T and a window long
        ChunkBufs c;
        Carve a(win, win_bytes);
        carve_chunked(a, m->cfg, B, W, W, &c);
        if (!a.ok) return fail(M2_E_WORKSPACE, "ragged vocoder: workspace too small (m2_ragged_workspace_bytes)");
        if ((rc = launch_ragged_gather(mel, mel_layout == 1, frames, B, T, M, c.mel, st))) return rc;
        const bool x3 = m->x3;
        const int redo = device_redo_word(m, x3);
        if ((rc = vocoder_run(m, c.mel, mel_layout, B, W, c.audio, c.voc, st, x3, redo))) return rc;
        if (redo < 0 && (rc = range_fallback(m, st, x3, [&] {
                             return vocoder_run(m, c.mel, mel_layout, B, W, c.audio, c.voc, st, false);
                         })))
            return rc;
        if ((rc = launch_ragged_scatter(c.audio, frames, B, T, out_audio, st))) return rc;
    }
    if ((rc = launch_ragged_tail(m->ragged_w, M, m->cfg.vocoder_channels, mel, mel_layout == 1, frames, B, T, out_audio,
                                 st)))
        return rc;
    return launch_ragged_zero(out_audio, frames, B, T, 64, st);
}

// The back half can run from a device-resident frame count with its grids
// sized for T_cap frames: the one-launch decoder layers with the mel
// projection fused into the last one, and the fused (unchunked) vocoder.
bool dev_back_ok(const m2_model* m, int32_t T_cap) {
    if (!sw().speculative) return false;  // M2_SPECULATIVE=0: host-side T only (A/B, tests)
    return T_cap > 0 && !tf_call_error(tf_call(m, true, TfSrc::Expand, false, true, false, 1, T_cap), sw()).code &&
           m->fused && !(m->chunk_frames > 0 && T_cap > m->chunk_frames);
}

// expansion to T frames + decoder + vocoder; dT: T is the capacity and the
// kernels take the frame count from the device word (dev_frames)
// rows: a ragged batch - utterance b has rows[b] frames of the T (ragged_supported)
int32_t back_run(const m2_model* m, int32_t B, int32_t S, int32_t T, const int32_t* dT, const void* front,
                 size_t front_bytes, float* out_mel, float* out_audio, void* workspace, size_t workspace_bytes,
                 void* stream, const int32_t* rows = nullptr) {
    M2_CHECK_ARG(m && B >= 0 && S >= 0 && T >= 0, "m2_inference_back: bad argument");
    if (B == 0 || T == 0) return M2_OK;
    M2_CHECK_ARG(out_mel && out_audio, "m2_inference_back: null output");
    const int H = m->cfg.hidden_dim;
    Carve a(const_cast<void*>(front), front_bytes);
    FrontBufs f;
    carve_front(a, B, S, H, &f);
    if (!a.ok) return fail(M2_E_WORKSPACE, "m2_inference_back: front buffer too small");
    // the regulated frames live after the decoder / vocoder scratch
    Carve w(workspace, workspace_bytes);
    Sizer sz_tf;
    carve_tf(sz_tf, B, T, H, m->cfg.num_heads, nullptr);
    const size_t scratch = std::max(sz_tf.off, vocoder_ws_bytes(m, B, T));
    (void)w.take<char>(scratch);
    float* reg = w.take<float>((size_t)B * T * H);
    const size_t win_bytes = rows ? ragged_extra_bytes(m, B) : 0;  // the ragged vocoder's window pass
    char* win = rows ? w.take<char>(win_bytes) : nullptr;
    if (!w.ok) return fail(M2_E_WORKSPACE, "m2_inference_back: workspace too small");
    int32_t rc;
    // frame expansion + decoder (the expansion fused into the first layer's launch)
    if ((rc = mel_decoder(m, reg, B, T, out_mel, workspace, scratch, static_cast<hipStream_t>(stream), f.enc, f.cum,
                          S, dT, rows)))
        return rc;
    if (rows) {  // the mel past each utterance's end is zero before the vocoder reads it
        if ((rc = launch_ragged_zero(out_mel, rows, B, T, m->cfg.mel_channels, static_cast<hipStream_t>(stream))))
            return rc;
        return vocoder_ragged(m, out_mel, 1, rows, B, T, out_audio, workspace, scratch, win, win_bytes, stream);
    }
    return vocoder_entry(m, out_mel, 1, B, T, out_audio, workspace, scratch, stream, dT);
}
}  // namespace

extern "C" {

int32_t m2_inference_front(const m2_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t S,
                           float scale, void* front, size_t front_bytes, void* workspace, size_t workspace_bytes,
                           int32_t* host_Tmax, void* stream) {
    M2_CHECK_ARG(host_Tmax, "m2_inference_front: bad argument");
    FrontBufs f;
    return front_run(m, ids, lengths, B, S, front, front_bytes, workspace, workspace_bytes,
                     static_cast<hipStream_t>(stream), &f, [&](FrontBufs& fb) {
                         return m2_length_regulator_count_sync(fb.dur, 0, scale, B, S, fb.cum, fb.tot, fb.tmax,
                                                               host_Tmax, stream);
                     });
}

int32_t m2_inference_front_dev(const m2_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t S,
                               float scale, void* front, size_t front_bytes, void* workspace, size_t workspace_bytes,
                               int32_t* dev_Tmax, void* stream) {
    M2_CHECK_ARG(dev_Tmax, "m2_inference_front_dev: null T_max word");
    hipStream_t st = static_cast<hipStream_t>(stream);
    FrontBufs f;
    const CountFuse cf{scale, dev_Tmax, m->cnt_ticket, nullptr, 0};
    return front_run(m, ids, lengths, B, S, front, front_bytes, workspace, workspace_bytes, st, &f,
                     [&](FrontBufs& fb) -> int32_t {
                         if (B == 0) {
                             M2_HIP(hipMemsetAsync(dev_Tmax, 0, sizeof(int32_t), st));
                             return M2_OK;
                         }
                         return launch_lr_count_sync(fb.dur, 0, scale, B, S, fb.cum, fb.tot, dev_Tmax,
                                                     m->cnt_ticket, nullptr, 0, st);
                     }, &cf);
}

int32_t m2_inference_back(const m2_model* m, int32_t B, int32_t S, int32_t T, const void* front, size_t front_bytes,
                          float* out_mel, float* out_audio, void* workspace, size_t workspace_bytes, void* stream) {
    return back_run(m, B, S, T, nullptr, front, front_bytes, out_mel, out_audio, workspace, workspace_bytes, stream);
}

int32_t m2_inference_dev_supported(const m2_model* m, int32_t T_cap) { return m && dev_back_ok(m, T_cap) ? 1 : 0; }

int32_t m2_inference_back_dev(const m2_model* m, int32_t B, int32_t S, int32_t T_cap, const int32_t* dev_T,
                              const void* front, size_t front_bytes, float* out_mel, float* out_audio,
                              void* workspace, size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(m && dev_T && T_cap > 0, "m2_inference_back_dev: bad argument");
    M2_CHECK_ARG(dev_back_ok(m, T_cap), "m2_inference_back_dev: this model's back half needs the host-side frame "
                                        "count (m2_inference_dev_supported is 0)");
    return back_run(m, B, S, T_cap, dev_T, front, front_bytes, out_mel, out_audio, workspace, workspace_bytes, stream);
}

int32_t m2_mel_decoder_ragged(const m2_model* m, const float* x, const int32_t* frames, int32_t B, int32_t T,
                              float* out_mel, void* workspace, size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(m && x && frames && out_mel && B >= 0 && T >= 0, "m2_mel_decoder_ragged: bad argument");
    if (int32_t rc = ragged_supported(m, true, false, "m2_mel_decoder_ragged")) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t rc = mel_decoder(m, const_cast<float*>(x), B, T, out_mel, workspace, workspace_bytes, st, nullptr, nullptr,
                             0, nullptr, frames);
    if (rc) return rc;
    return launch_ragged_zero(out_mel, frames, B, T, m->cfg.mel_channels, st);
}

int32_t m2_vocoder_ragged(const m2_model* m, const float* mel, int32_t mel_layout, const int32_t* frames, int32_t B,
                          int32_t T, float* out_audio, void* workspace, size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(m && mel && frames && out_audio && B >= 0 && T >= 0, "m2_vocoder_ragged: bad argument");
    M2_CHECK_ARG(mel_layout == 0 || mel_layout == 1, "m2_vocoder_ragged: mel_layout must be 0 or 1");
    if (int32_t rc = ragged_supported(m, false, true, "m2_vocoder_ragged")) return rc;
    if (B == 0 || T == 0) return M2_OK;
    // the window pass's scratch is the end of the workspace
    const size_t extra = ragged_extra_bytes(m, B);
    if (!workspace || workspace_bytes < extra) return fail(M2_E_WORKSPACE, "m2_vocoder_ragged: workspace too small");
    const size_t main_bytes = (workspace_bytes - extra) / 256 * 256;
    return vocoder_ragged(m, mel, mel_layout, frames, B, T, out_audio, workspace, main_bytes,
                          static_cast<char*>(workspace) + main_bytes, workspace_bytes - main_bytes, stream);
}

size_t m2_ragged_workspace_bytes(const m2_model* m, int32_t B) {
    if (!m || B < 0) return 0;
    return ragged_extra_bytes(m, B);
}

int32_t m2_inference_back_ragged(const m2_model* m, int32_t B, int32_t S, int32_t T, const void* front,
                                 size_t front_bytes, float* out_mel, float* out_audio, int32_t* out_frames,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(m && B >= 0 && S >= 0 && T >= 0, "m2_inference_back_ragged: bad argument");
    if (int32_t rc = ragged_supported(m, true, true, "m2_inference_back_ragged")) return rc;
    if (B == 0 || T == 0) return M2_OK;
    M2_CHECK_ARG(out_mel && out_audio && out_frames, "m2_inference_back_ragged: null output");
    hipStream_t st = static_cast<hipStream_t>(stream);
    Carve a(const_cast<void*>(front), front_bytes);
    FrontBufs f;
    carve_front(a, B, S, m->cfg.hidden_dim, &f);
    if (!a.ok) return fail(M2_E_WORKSPACE, "m2_inference_back_ragged: front buffer too small");
    int32_t rc;
    if ((rc = launch_ragged_count(f.tot, B, out_frames, st))) return rc;
    return back_run(m, B, S, T, nullptr, front, front_bytes, out_mel, out_audio, workspace, workspace_bytes, stream,
                    out_frames);
}

int32_t m2_frames_wait(const m2_model* m, void* stream, int32_t* host_T) {
    M2_CHECK_ARG(m && host_T, "m2_frames_wait: bad argument");
    M2_CHECK_ARG(m->fpost_seq > 0, "m2_frames_wait: no m2_inference_back_dev call to wait for");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int32_t seq = m->fpost_seq;
    for (unsigned i = 1;; ++i) {
        if (__atomic_load_n(m->fpost_host, __ATOMIC_ACQUIRE) == seq) break;
        if ((i & 1023) == 0) {
            const hipError_t e = hipStreamQuery(st);
            if (e == hipSuccess) {
                if (__atomic_load_n(m->fpost_host, __ATOMIC_ACQUIRE) == seq) break;
                return fail(M2_E_INTERNAL, "m2_frames_wait: stream idle but T not posted");
            }
            if (e != hipErrorNotReady) return hip_status(e, "m2_frames_wait");
        }
        _mm_pause();
    }
    *host_T = __atomic_load_n(m->fpost_host + 1, __ATOMIC_RELAXED);
    return M2_OK;
}

int32_t m2_inference(const m2_model* m, const int64_t* ids, const int64_t* lengths, int32_t B, int32_t S, float scale,
                     void* front, size_t front_bytes, void* workspace, size_t workspace_bytes, float* mel_buf,
                     size_t mel_cap, float* audio_buf, size_t audio_cap, int32_t* host_T, int32_t* launched,
                     void* stream) {
    M2_CHECK_ARG(m && host_T && launched, "m2_inference: bad argument");
    *launched = 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // The capacity the caller's buffers give: with one, the back half is
    // enqueued right behind the count kernel, before the host reads T_max,
    // its kernels taking the frame count from the device (dev_frames) - the
    // host wait overlaps the decoder instead of idling the GPU.
    int32_t cap = 0;
    if (B > 0 && mel_buf && audio_buf) {
        const size_t c1 = mel_cap / ((size_t)B * m->cfg.mel_channels), c2 = audio_cap / ((size_t)B * 64);
        cap = (int32_t)std::min<size_t>(std::min(c1, c2), (size_t)kMaxFrames);
        if (cap > 0 && m2_inference_workspace_bytes(m, B, S, cap) > workspace_bytes) cap = 0;
    }
    const bool spec = cap > 0 && S > 0 && dev_back_ok(m, cap);
    int32_t rc, tmax = 0;
    FrontBufs f;
    if (!spec) {
        if ((rc = m2_inference_front(m, ids, lengths, B, S, scale, front, front_bytes, workspace, workspace_bytes,
                                     &tmax, stream)))
            return rc;
    } else {
        int dev = 0;
        if ((rc = stream_device(st, &dev))) return rc;
        std::lock_guard<std::mutex> lk(g_mb_mu);
        LrMailbox* mb = nullptr;
        if ((rc = mailbox_for(dev, st, &mb))) return rc;
        mb->seq = mb->seq == INT_MAX ? 1 : mb->seq + 1;
        const int32_t seq = mb->seq;
        const CountFuse cf{scale, nullptr, mb->ticket, mb->dev, seq};
        if ((rc = front_run(m, ids, lengths, B, S, front, front_bytes, workspace, workspace_bytes, st, &f,
                            [&](FrontBufs& fb) {
                                return launch_lr_count_sync(fb.dur, 0, scale, B, S, fb.cum, fb.tot, fb.tmax, mb->ticket,
                                                            mb->dev, seq, st);
                            }, &cf)))
            return rc;
        if ((rc = back_run(m, B, S, cap, f.tmax, front, front_bytes, mel_buf, audio_buf, workspace, workspace_bytes,
                           stream)))
            return rc;
        if ((rc = mailbox_wait(mb, seq, st, &tmax, "m2_inference"))) return rc;
        M2_CHECK_SHAPE(tmax <= kMaxFrames, "length regulator: an utterance's frame count exceeds 2^24 (the "
                                           "durations times duration_scale are out of range)");
    }
    const int32_t T = std::max(1, tmax);  // tts_model.py:158-160
    *host_T = T;
    if (spec) {  // done unless T outgrew the capacity (then the launches did nothing)
        *launched = T <= cap ? 1 : 0;
        return M2_OK;
    }
    const size_t need_mel = (size_t)B * T * m->cfg.mel_channels, need_audio = (size_t)B * 64 * T;
    if (!mel_buf || !audio_buf || need_mel > mel_cap || need_audio > audio_cap ||
        m2_inference_workspace_bytes(m, B, S, T) > workspace_bytes)
        return M2_OK;  // the caller allocates for T and calls m2_inference_back
    if ((rc = m2_inference_back(m, B, S, T, front, front_bytes, mel_buf, audio_buf, workspace, workspace_bytes,
                                stream)))
        return rc;
    *launched = 1;
    return M2_OK;
}

size_t m2_inference_workspace_bytes(const m2_model* model, int32_t B, int32_t S, int32_t T) {
    if (!model || B < 0 || S < 0 || T < 0) return 0;
    const int H = model->cfg.hidden_dim;
    Sizer a, b, d;
    carve_tf(a, B, S, H, model->cfg.num_heads, nullptr);
    carve_tf(b, B, T, H, model->cfg.num_heads, nullptr);
    d.off = std::max(b.off, vocoder_ws_bytes(model, B, T));
    (void)d.take<float>((size_t)B * T * H);
    return std::max(a.off, d.off) + 256;
}

int32_t m2_vocoder_path(const m2_model* m) {
    if (!m) return -1;
    return m->x3 ? 2 : (m->fused ? 1 : 0);
}

int32_t m2_transformer_path(const m2_model* m) {
    if (!m) return -1;
    if (!(m->tfused && !m->att_f32)) return 0;
    for (const auto* st : {&m->enc, &m->dec})
        for (const m2_layer_w& L : *st)
            if (L.wide_scores) return 2;
    return 1;
}

int32_t m2_debug_transformer_form(const m2_model* m, int32_t stack) {
    M2_CHECK_ARG(m && (stack == 0 || stack == 1), "m2_debug_transformer_form: bad argument");
    return tf_form(tf_call(m, stack != 0, TfSrc::X, false, false, false, 1, 1), sw());
}

int32_t m2_debug_transformer_plan(const m2_model* m, int32_t stack, int32_t B, int32_t N, int32_t masked,
                                  int32_t source, int32_t device_T, int32_t ragged, char* out, size_t cap) {
    M2_CHECK_ARG(m && (stack == 0 || stack == 1) && B >= 0 && N >= 0 && source >= 0 && source <= 2,
                 "m2_debug_transformer_plan: bad argument");
    // the calls the entry points make: the encoder embeds (source 0 plans the same layers on given rows)
    // and may be masked; the decoder takes rows or the expansion, a device frame count or ragged rows
    M2_CHECK_ARG(stack == 1 ? (!masked && source != 1) : (source != 2 && !device_T && !ragged),
                 "m2_debug_transformer_plan: no entry point makes this call (encoder: source 0 | 1, masked; decoder: "
                 "source 0 | 2, device_T, ragged)");
    const TfCall c = tf_call(m, stack != 0, (TfSrc)source, masked != 0, device_T != 0, ragged != 0, B, N);
    return plan_transformer(c, sw()).print(out, cap);
}

int32_t m2_profile_enable(m2_model* m, int32_t capacity) {
    M2_CHECK_ARG(m && capacity >= 0, "m2_profile_enable: bad argument");
    m2_profile_disable(m);
    for (int i = 0; i < capacity * kVocKernels; ++i) {
        hipEvent_t a, b;
        // No system-scope fence: a default event writes back and invalidates
        // L2 at every record, which costs the next kernel its warm weights.
        M2_HIP(hipEventCreateWithFlags(&a, hipEventDisableSystemFence));
        M2_HIP(hipEventCreateWithFlags(&b, hipEventDisableSystemFence));
        m->prof_begin.push_back(a);
        m->prof_end.push_back(b);
    }
    m->prof_calls = 0;
    m->prof_seen = 0;
    return M2_OK;
}

int32_t m2_profile_read(m2_model* m, float* ms_out, int32_t capacity, int32_t* n_out) {
    M2_CHECK_ARG(m && ms_out && n_out, "m2_profile_read: bad argument");
    const int n = std::min<int>(capacity, m->prof_calls * kVocKernels);
    for (int i = 0; i < n; ++i) {
        ms_out[i] = -1.f;  // kernel not selected
        if (!((m->prof_mask >> (i % kVocKernels)) & 1u)) continue;
        M2_HIP(hipEventSynchronize(m->prof_end[i]));
        M2_HIP(hipEventElapsedTime(&ms_out[i], m->prof_begin[i], m->prof_end[i]));
    }
    *n_out = n;
    m->prof_calls = 0;
    return M2_OK;
}

int32_t m2_profile_select(m2_model* m, uint32_t kernel_mask) {
    M2_CHECK_ARG(m, "m2_profile_select: null model");
    m->prof_mask = kernel_mask;
    return M2_OK;
}

int32_t m2_profile_stride(m2_model* m, int32_t stride) {
    M2_CHECK_ARG(m && stride >= 1, "m2_profile_stride: bad argument");
    m->prof_stride = stride;
    m->prof_seen = 0;
    return M2_OK;
}

int32_t m2_profile_disable(m2_model* m) {
    if (!m) return M2_OK;
    for (auto e : m->prof_begin) (void)hipEventDestroy(e);
    for (auto e : m->prof_end) (void)hipEventDestroy(e);
    m->prof_begin.clear();
    m->prof_end.clear();
    m->prof_calls = 0;
    return M2_OK;
}

}  // extern "C"
