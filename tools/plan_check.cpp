// The handle's creation plan (csrc/m2_model.h) run on the CPU: no GPU is
// initialised.  Built with the host code under ASan + UBSan by
//   make -C m2-tts_amd/csrc plan_check
// Fills the stage1 and stage2 weight tables from a fixed LCG in +-0.1, plans,
// and prints every decision and pack size; then once more with one vocoder
// and one transformer weight outside the f16 range.  Exit status 1 when a
// flag is not the expected one.
// Every buffer the plan produces is also hashed (64-bit FNV-1a over its bytes)
// and compared with the value recorded before the pipelined vocoder kernels'
// packers were merged into vocoder_pipe.h: the LCG weights are non-zero
// everywhere, so a wrong slot, a lost duplicate zeroing or a changed summation
// order in a packer changes a hash.
// The training losses' plans (csrc/losses_plan.h) run here too: the discriminator
// calls' sizes and workspace layout against the formulas they replaced, and the
// backward kernels' launch plans against their limits.
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "losses_plan.h"
#include "m2_model.h"
#include "vocoder_pipe.h"

using namespace m2;

static int g_bad = 0;

static void expect(const char* what, bool got, bool want) {
    std::printf(" %s=%d%s", what, (int)got, got == want ? "" : "(UNEXPECTED)");
    g_bad += got != want;
}

template <typename T>
static uint64_t fnv1a(const std::vector<T>& v) {
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

// [case: stage1, stage2, stage1 7e4, stage2 7e4][tail, mid, split, f32, dur bn, dur pack, dur split, tf packs]
static const uint64_t kHashes[4][8] = {
    {0xf701b5b22ef7a4ceull, 0xcef17728435c7665ull, 0x61ef7faa2f05b383ull, 0xa71c9fe680c81899ull,
     0x8080e8e153256022ull, 0x9d234fbe127e3186ull, 0x9aa908de7230946full, 0x5db086f6f822ae64ull},
    {0xfdb0fb49b660bc54ull, 0xcbf29ce484222325ull, 0x879f897dba138908ull, 0x37c53b3319b6cad2ull,
     0x9f20bc6f3901c58bull, 0x15836341343d91f7ull, 0xfbd64d10a43db258ull, 0xfe1f65a7662f23f4ull},
    {0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0x30e4dc780eb7a4b3ull,
     0x8080e8e153256022ull, 0x9d234fbe127e3186ull, 0x9aa908de7230946full, 0x487d7fa11a668f7bull},
    {0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xe7fadbaeb39b0483ull,
     0x9f20bc6f3901c58bull, 0x15836341343d91f7ull, 0xfbd64d10a43db258ull, 0x2f479c92320031d9ull},
};

static void expect_hash(const char* what, uint64_t got, uint64_t want) {
    std::printf(" %s=0x%016llxull%s", what, (unsigned long long)got, got == want ? "" : "(UNEXPECTED)");
    g_bad += got != want;
}

static void check(int idx, const char* stage, const m2_config& c, bool huge) {
    const std::vector<WSpec> table = weight_table(c);
    const BufLayout lay = buf_layout(table, c);
    HostWeights w{table, lay, std::vector<float>(lay.bn_off, 0.f)};
    uint32_t lcg = 12345u;
    for (size_t i = 0; i < table.size(); ++i) {
        if (table[i].is_int64) continue;
        const std::string& n = table[i].name;
        const bool var = n.size() > 11 && n.compare(n.size() - 11, 11, "running_var") == 0;
        for (int64_t k = 0; k < table[i].numel; ++k) {
            lcg = lcg * 1664525u + 1013904223u;
            const float v = ((lcg >> 8) / 16777216.0f - 0.5f) * 0.2f;
            w.raw[lay.off[i] + k] = var ? 1.0f + v : v;
        }
    }
    if (huge) {
        w.raw[lay.off[w.index("vocoder.resblocks.3.conv1.weight")]] = 7e4f;
        w.raw[lay.off[w.index("text_encoder.layers.0.ffn.linear1.weight")]] = 7e4f;
    }
    const bool s1 = c.mel_channels == 64;
    const Switches& s = sw();
    const DurationPlan d = plan_duration(w, c);
    const TransformerPlan t = plan_transformer(w, c, s);
    VocoderPlan v;
    plan_vocoder(w, c, s, &v);
    std::printf("%s %s:", stage, huge ? "7e4 " : "+-0.1");
    expect("dur_split", d.dur_split, true);
    expect("tfused", t.tfused, !huge);
    expect("att_f32", t.att_f32, huge);
    expect("fused", v.fused, true);
    expect("f32_parts_ok", v.f32.slots.size() == (s1 ? 32u : 29u), true);  // the composed head's three parts among them
    expect("x3", v.x3, !huge);
    expect("split_parts_ok", v.split.slots.size() == (huge ? 0u : 16u), true);
    expect("tailp", !v.tail.buf.empty(), !huge);
    expect("midp", !v.mid.buf.empty(), !huge && s1);
    std::printf("\n  sizes: raw %zu buf %zu | dur %zu %zu %zu | tf %zu packs %zu | f32 %zu in %zu | split %zu in %zu | "
                "tail %zu bias@%zu | mid %zu bias@%zu\n",
                lay.bn_off, lay.total, d.bn.size(), d.pack.size(), d.split.size(), t.at.size(), t.packs.size(),
                v.f32.host.size(), v.f32.slots.size(), v.split.host.size(), v.split.slots.size(), v.tail.buf.size(),
                v.tail.bias_at, v.mid.buf.size(), v.mid.bias_at);
    std::printf("  hashes:");
    const uint64_t* hx = kHashes[idx];
    expect_hash("tail", fnv1a(v.tail.buf), hx[0]);
    expect_hash("mid", fnv1a(v.mid.buf), hx[1]);
    expect_hash("split", fnv1a(v.split.host), hx[2]);
    expect_hash("f32", fnv1a(v.f32.host), hx[3]);
    std::printf("\n         ");
    expect_hash("dur_bn", fnv1a(d.bn), hx[4]);
    expect_hash("dur_pack", fnv1a(d.pack), hx[5]);
    expect_hash("dur_split", fnv1a(d.split), hx[6]);
    expect_hash("tf_packs", fnv1a(t.packs), hx[7]);
    std::printf("\n");
    // every slot inside its buffer, at the buffer's alignment
    for (const auto& sl : v.f32.slots) g_bad += sl.second % 64 != 0 || sl.second > v.f32.host.size();
    for (const auto& sl : v.split.slots) g_bad += sl.second % 128 != 0 || sl.second > v.split.host.size();
}

// The strip-length loop as the three launchers carried it before pipe::pick_strip
// (verbatim; kept here only as the reference of the comparison below).
static int old_strip(int L, int B, int nmin, int per_round, int extra) {
    int nch = 0;
    const long chunks = cdiv(L, 16);
    long best = -1;
    for (int n = nmin; n <= 256; ++n) {
        const long wgs = (long)cdiv((int)chunks, n) * B, rounds = (wgs + per_round - 1) / per_round,
                   cost = rounds * (n + extra);
        if (best < 0 || cost < best) best = cost, nch = n;
    }
    return nch;
}

// pick_strip against the old loop: 1..3000 chunks, B in {1, 8, 16, 32}, the
// constants of tailp (6 and 7 layers), tailp2 (6 and 7) and midp.
static void check_strips() {
    const int sets[5][3] = {{8, 768, 7}, {8, 768, 8}, {8, 256, 6}, {8, 256, 7}, {4, 256, 4}};
    int diff = 0;
    for (const auto& k : sets)
        for (const int B : {1, 8, 16, 32})
            for (int chunks = 1; chunks <= 3000; ++chunks)
                diff += pipe::pick_strip(chunks, B, k[0], k[1], k[2]) != old_strip(16 * chunks, B, k[0], k[1], k[2]);
    std::printf("pick_strip:");
    expect("same_as_old_loop", diff == 0, true);
    std::printf("\n");
}

// ---- the training losses' plans (csrc/losses_plan.h) ---------------------------------

// The discriminator calls' sizes as losses.hip carried them before loss::disc_plan and
// loss::carve_disc: step_plan, the max_chunks expression and the three byte formulas (verbatim,
// over a stand-in for the handle; kept here only as the reference of the comparison below).
struct old_disc {
    int n_scales;
    int scales[loss::kMaxScales];
    size_t slice_bytes;
};
using loss::disc_floats;
using loss::disc_lengths;
using loss::dw_plan;
using loss::kDisc;
using loss::kLayers;

static size_t disc_floats_max(const old_disc* d, int L) {
    size_t n = 0;
    for (int s = 0; s < d->n_scales; ++s) n = std::max(n, disc_floats(L, d->scales[s]));
    return n;
}

static int slice_of(const old_disc* d, size_t floats_per_utt, int copies, int B) {
    const size_t per = std::max<size_t>(1, floats_per_utt * copies * sizeof(float));
    const size_t n = d->slice_bytes / per;
    return (int)std::max<size_t>(1, std::min<size_t>(n, (size_t)std::max(B, 1)));
}

struct StepPlan {
    size_t per = 0;      // floats of the seven maps of one utterance and side
    size_t cot = 0;      // floats of the widest map of one utterance: each of the two cotangent buffers
    size_t pooled = 0;   // floats of the pooled audio of one utterance (scales above 1)
    size_t part = 0;     // floats of the split-K partials
    int nbs = 1, max_chunks = 1;
};

static StepPlan step_plan(const old_disc* d, int B, int L) {
    StepPlan p;
    p.per = disc_floats_max(d, L);
    for (int s = 0; s < d->n_scales; ++s) {
        int len[kLayers];
        if (!disc_lengths(L, d->scales[s], len)) continue;
        for (int i = 0; i < kLayers; ++i) p.cot = std::max(p.cot, align_up((size_t)kDisc[i].Cout * len[i], 64));
        if (d->scales[s] > 1) p.pooled = std::max(p.pooled, align_up((size_t)(L / d->scales[s]), 64));
    }
    p.nbs = slice_of(d, p.per, 2, B);  // m2_disc_losses's slices: the bound counts the maps of both sides
    p.max_chunks = cdiv((int)std::min<size_t>(p.per, (size_t)1 << 30), loss::kRedChunk) + 1;
    for (int s = 0; s < d->n_scales; ++s) {
        int l = L / d->scales[s];
        if (l < 1) continue;
        // the last slice may be shorter, and fewer utterances never take more partials
        for (int i = 0; i < kLayers; ++i) {
            p.part = std::max(p.part, dw_plan(kDisc[i], p.nbs, l).part_floats);
            l = loss::conv_out_len(l, kDisc[i]);
        }
    }
    return p;
}

static size_t old_forward_bytes(const old_disc* d, int B, int L) {
    const size_t per = disc_floats_max(d, L);
    return (size_t)slice_of(d, per, 1, B) * per * sizeof(float) + 256 * (kLayers + 1);
}

static size_t old_losses_bytes(const old_disc* d, int B, int L) {
    const size_t per = disc_floats_max(d, L);
    const int nbs = slice_of(d, per, 2, B);
    const size_t chunks = (size_t)cdiv((int)std::min<size_t>(per, (size_t)1 << 30), loss::kRedChunk) + 1;
    return (size_t)nbs * per * 2 * sizeof(float) + (size_t)nbs * kLayers * chunks * loss::kRedPart * sizeof(double) +
           256 * 4;
}

static size_t old_step_bytes(const old_disc* d, int B, int L) {
    const StepPlan p = step_plan(d, B, L);
    return (size_t)p.nbs * (2 * p.per + 2 * p.cot + p.pooled) * sizeof(float) + p.part * sizeof(float) +
           (size_t)p.nbs * kLayers * p.max_chunks * loss::kRedPart * sizeof(double) + 256 * 8;
}

static size_t old_gen_step_bytes(const old_disc* d, int B, int L) {
    const StepPlan p = step_plan(d, B, L);
    return (size_t)p.nbs * (2 * p.per + 2 * p.cot) * sizeof(float) +
           (size_t)p.nbs * kLayers * p.max_chunks * loss::kRedPart * sizeof(double) + 256 * 8;
}

// disc_plan and carve_disc against the old code, for every mode: the sizes a mode uses are the
// old ones (the others are 0), the byte count is the old one less the slack it no longer needs,
// and a Carve over exactly Sizer::off bytes of host memory places every buffer inside it, apart
// from the others, while one byte fewer is refused.
static void check_disc_plans() {
    int fields = 0, bytes = 0, carves = 0, carved = 0, order = 0;
    for (const int B : {1, 2, 3, 32, 1000})
        for (const int L : {4, 1025, 3000, 32000, 1 << 20})
            for (const size_t slice : {loss::kSliceBytes, (size_t)8 << 20, (size_t)1}) {
                const old_disc d{3, {1, 2, 4}, slice};
                const StepPlan ref = step_plan(&d, B, L);
                size_t count[4];
                for (int m = 0; m < 4; ++m) {
                    const loss::DiscMode mode = (loss::DiscMode)m;
                    const loss::DiscPlan p = loss::disc_plan(d.scales, d.n_scales, d.slice_bytes, B, L, mode);
                    const bool rows = mode != loss::DISC_FORWARD, steps = mode >= loss::DISC_GEN_STEP;
                    size_t layers = 0;  // m2_disc_forward lays the layers' widest maps out inside `per`
                    for (int i = 0; i < kLayers; ++i) layers += align_up(p.layer[i], 64);
                    fields += p.per != ref.per || layers != p.per || p.sides != (rows ? 2 : 1) ||
                              p.nbs != (rows ? ref.nbs : slice_of(&d, ref.per, 1, B)) ||
                              p.max_chunks != (rows ? ref.max_chunks : 0) || p.cot != (steps ? ref.cot : 0) ||
                              p.pooled != (mode == loss::DISC_STEP ? ref.pooled : 0) ||
                              p.part != (mode == loss::DISC_STEP ? ref.part : 0);
                    Sizer s;
                    loss::carve_disc(s, p, nullptr);
                    count[m] = s.off + 256;
                    const size_t old = mode == loss::DISC_FORWARD    ? old_forward_bytes(&d, B, L)
                                       : mode == loss::DISC_LOSSES   ? old_losses_bytes(&d, B, L)
                                       : mode == loss::DISC_GEN_STEP ? old_gen_step_bytes(&d, B, L)
                                                                     : old_step_bytes(&d, B, L);
                    bytes += count[m] > old || old - count[m] >= 2048;
                    if (s.off > ((size_t)64 << 20)) continue;  // the small cases: a real allocation
                    ++carved;
                    std::vector<char> mem(s.off);
                    Carve c(mem.data(), mem.size()), less(mem.data(), mem.size() - 1);
                    loss::DiscBufs b, none;
                    loss::carve_disc(c, p, &b);
                    loss::carve_disc(less, p, &none);
                    const size_t act = (size_t)p.nbs * p.per * sizeof(float);
                    const size_t cot = (size_t)p.nbs * p.cot * sizeof(float);
                    const std::pair<const void*, size_t> bufs[] = {
                        {b.act[0], act},
                        {b.act[1], rows ? act : 0},
                        {b.dpart, (size_t)p.nbs * kLayers * p.max_chunks * loss::kRedPart * sizeof(double)},
                        {b.cot[0], cot},
                        {b.cot[1], cot},
                        {b.pooled, (size_t)p.nbs * p.pooled * sizeof(float)},
                        {b.part, p.part * sizeof(float)}};
                    bool good = c.ok && !less.ok;
                    const char* end = mem.data();  // carved in this order: each begins at or after the last one's end
                    for (const auto& bf : bufs) {
                        const char* at = static_cast<const char*>(bf.first);
                        if (bf.second == 0) {
                            good = good && at == nullptr;
                            continue;
                        }
                        good = good && at != nullptr && at >= end && at + bf.second <= mem.data() + mem.size();
                        end = at + bf.second;
                    }
                    carves += !good;
                }
                order += !(count[loss::DISC_LOSSES] < count[loss::DISC_GEN_STEP] &&
                           count[loss::DISC_GEN_STEP] < count[loss::DISC_STEP]);
            }
    std::printf("disc_plan:");
    expect("sizes_same_as_old", fields == 0, true);
    expect("bytes_within_2KiB_below_old", bytes == 0, true);
    expect("carve_exact_inside_disjoint", carves == 0 && carved > 0, true);
    expect("losses_lt_gen_step_lt_step", order == 0, true);
    std::printf(" (%d carved)\n", carved);
}

// dw_plan, dx_mfma_ok and audio_bwd_ok over the discriminators' layers at the input lengths of the
// GPU tests' cases (audio of 2624 and 1001 samples at scales 1, 2, 4; 1; 103) and over the other
// geometries those tests run: every plan that is accepted launches within the limits.
static void check_geometries() {
    struct Geo {
        loss::ConvGeo g;
        std::vector<int> L;
    };
    std::vector<Geo> geos;
    for (int i = 0; i < kLayers; ++i) {
        Geo e{kDisc[i], {1, 103}};
        for (const int L : {2624, 1001})
            for (const int scale : {1, 2, 4}) {
                int len[kLayers];
                disc_lengths(L, scale, len);
                e.L.push_back(i == 0 ? L / scale : len[i - 1]);
            }
        geos.push_back(e);
    }
    geos.push_back({{6, 10, 4, 3, 2, 2}, {50}});
    geos.push_back({{6, 10, 4, 3, 0, 2}, {50}});
    geos.push_back({{16, 16, 3, 2, 0, 1}, {150}});
    geos.push_back({{16, 32, 2, 3, 0, 1}, {200}});
    geos.push_back({{36, 48, 7, 3, 5, 4}, {70}});
    geos.push_back({{24, 40, 5, 1, 2, 1}, {6}});
    int bad = 0, mfma_dw = 0, mfma_dx = 0;
    for (const Geo& e : geos) {
        const loss::ConvGeo& g = e.g;
        const loss::WStride raw = loss::w_stride(g, false), packed = loss::w_stride(g, true);
        const long long Cg = g.Cin / g.groups;
        bad += raw.sCo != Cg * g.k || raw.sCi != g.k || raw.sK != 1 || packed.sCo != 1 || packed.sCi != g.Cout ||
               packed.sK != Cg * g.Cout;
        if (loss::dx_mfma_ok(g)) {
            ++mfma_dx;
            bad += loss::dx_lds_bytes(g) > (size_t)loss::kMaxLds || loss::dx_grid_y(g) > loss::kMaxGrid ||
                   loss::dx_grid_y(g) < 1;
        }
        for (const int L : e.L)
            for (const int nb : {1, 2, 3, 32, 1000}) {
                const loss::DwPlan p = dw_plan(g, nb, L);
                const size_t n = (size_t)g.Cout * Cg * g.k;
                if (!p.mfma) {
                    bad += p.part_floats != 0;
                    continue;
                }
                ++mfma_dw;
                const long long chunks = (long long)nb * cdiv(loss::conv_out_len(L, g), loss::kTc);
                bad += p.lds > (size_t)loss::kMaxLds || p.blocks < 1 || p.blocks > loss::kMaxGrid ||
                       cdiv(g.Cout, 16) > loss::kMaxGrid || p.splits < 1 || p.splits > loss::kMaxSplits ||
                       p.nciB < 1 || p.nciB * g.k > loss::kDwCols || (long long)p.cps * p.splits < chunks ||
                       p.part_floats < (size_t)p.splits * n;
            }
    }
    const loss::ConvGeo& first = kDisc[0];
    const bool audio = loss::audio_bwd_ok(first.Cout, first.k) &&
                       loss::audio_lds_bytes(first.Cout, first.k) <= (size_t)loss::kMaxLds;
    std::printf("loss geometries:");
    expect("accepted_plans_within_limits", bad == 0 && mfma_dw > 0 && mfma_dx > 0, true);
    expect("first_layer_audio_bwd_ok", audio, true);
    expect("audio_bwd_refuses_wide_weights", !loss::audio_bwd_ok(1024, 41) && !loss::audio_bwd_ok(1, 1 << 13), true);
    std::printf(" (%d dw plans, %d dx geometries on the MFMA)\n", mfma_dw, mfma_dx);
}

int main() {
    check_strips();
    check_disc_plans();
    check_geometries();
    const m2_config stage1{256, 64, 64, 2, 2, 2, 128, 1000}, stage2{256, 96, 80, 3, 3, 2, 256, 1000};
    for (const bool huge : {false, true}) {
        check(2 * huge, "stage1", stage1, huge);
        check(2 * huge + 1, "stage2", stage2, huge);
    }
    std::printf("plan_check: %d unexpected\n", g_bad);
    return g_bad ? 1 : 0;
}
