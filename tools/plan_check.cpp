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
// The vocoder's launch plan (csrc/vocoder_launch.h) runs here too: plan_vocoder_launch against
// the decision rules the launchers carried before it (old_* below), over a sweep of calls, switch
// tables and workgroup-slot counts, with the plans' invariants and three pinned lines.
// The transformer stacks' launch plan (csrc/transformer_plan.h) likewise: plan_transformer against the
// rules the drivers and launchers carried before it (old_transformer), over a sweep of handles, calls
// and switch tables, with the plans' invariants and three pinned lines (check_transformer_plan).
// The training losses' plans (csrc/losses_plan.h) run here too: the discriminator
// calls' sizes and workspace layout against the formulas they replaced, and the
// backward kernels' launch plans against their limits, and the spectral backward's
// workspace carve against its frame count.
// The decoder's gradient plan (csrc/decoder_grad_plan.h) is checked the same way (check_decoder_grad).
// The text encoder's gradient plan (csrc/encoder_grad_plan.h) likewise (check_encoder_grad), with the
// embedding's split over the positions.
// The duration predictor's gradient plan (csrc/duration_grad_plan.h) likewise (check_duration_grad).
// The vocoder's gradient plan (csrc/vocoder_grad_plan.h) runs here too: the tape and the backward's
// workspace against a plain restatement of their formulas, the carved regions against each other,
// and every launch row against the LDS and grid limits.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "losses_plan.h"
#include "m2_model.h"
#include "transformer_plan.h"
#include "decoder_grad_plan.h"
#include "duration_grad_plan.h"
#include "encoder_grad_plan.h"
#include "vocoder_grad_plan.h"
#include "vocoder_launch.h"
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

// ---- the vocoder's launch plan (csrc/vocoder_launch.h) -------------------------------

// The launch decisions as vocoder_run, x3::run<Cfg>, the three pipelined launchers and
// launch_vocoder_fused / s1_fused carried them before plan_vocoder_launch (transcribed, sw() made
// an argument; kept here only as the reference of the comparison below).
static const char* old_headmid_excluded(const VocCall& w, const Switches& s, bool comp, bool s1) {
    if (!s.headmid) return "M2_HEADMID=0";
    if (!s1) return "not the stage1 shapes";
    if (w.device_T) return "the frame count is on the device: the grid covers the capacity";
    if (!w.mp || !w.hc || !comp) return "no split packs of the composed head and the pipelined mid (or M2_HEAD_INCONV)";
    if (s.midp_nch > 0) return "M2_MIDP_NCH forces the mid's strip length";
    if (w.prof_slots & 3u) return "events around the head or the mid: the fused launch has no boundary between them";
    return nullptr;
}
static long old_rounds_of(long n, long slots) { return (n + slots - 1) / slots; }

struct OldSplit {
    const char* why = nullptr;  // headmid_excluded
    int n = 0, S = 0, nch = 0;  // headmid
    int head_tf = 0, head_waves = 0;
    bool comp = false, alt_mid = false, alt_tail = false;
    int midp_nch = 0;                  // 0: not the pipelined mid
    int tail_nl = 0, tail_nch = 0;     // 0: not a pipelined tail
    int redo = 0;                      // 0 none, 1 in the tail, 2 guarded launch, 3 host fallback
};

static OldSplit old_split(const VocCall& w, const Switches& s, const VocSlots& sl) {
    OldSplit o;
    const bool S1 = w.M == 64, S2 = w.M == 80;
    const int B = w.B, T = w.T;
    // vocoder_run / vocoder_entry: the three redo forms
    if (w.redo >= 0) o.redo = w.redo_w && !s.redo_launch ? 1 : 2;
    else if (w.range_policy == 1) o.redo = 3;
    // x3::run<Cfg>
    if (S2) {
        if (!w.mp && s.s2_mid_alt >= 0)
            o.alt_mid = s.s2_mid_alt == 1;
        else if (!w.mp)
            o.alt_mid = old_rounds_of((long)cdiv(4 * T, 33) * B, sl.mid_alt) * 1.20 <
                        (double)old_rounds_of((long)cdiv(4 * T, 30) * B, sl.mid);
        if (!w.tp && !w.tp2)
            o.alt_tail = old_rounds_of((long)cdiv(16 * T, 125) * B, sl.tail_alt) * 1.075 <
                         (double)old_rounds_of((long)cdiv(16 * T, 120) * B, sl.tail);
    }
    // the tail lambda: launch_vocoder_tailp2 / launch_vocoder_tailp
    if (w.tp2) {
        const bool seven = s.tailp2_seven;
        o.tail_nl = seven ? 7 : 6;
        int nch = s.tailp2_nch > 0 ? std::min(s.tailp2_nch, 4096) : 0;
        if (!nch) nch = old_strip(16 * T, B, 8, 256, o.tail_nl);
        o.tail_nch = nch;
    } else if (w.tp) {
        o.tail_nl = s.tailp_seven ? 7 : 6;
        int nch = s.tailp_nch > 0 ? std::min(s.tailp_nch, 4096) : 0;
        if (!nch) nch = old_strip(16 * T, B, 8, 768, o.tail_nl + 1);
        o.tail_nch = nch;
    }
    o.comp = w.hc && !s.head_inconv;
    if (S1) {
        o.why = old_headmid_excluded(w, s, o.comp, S1);
        if (!o.why) {
            o.n = cdiv(4 * T, 4 * 63 - 2), o.S = cdiv(4 * T, o.n), o.nch = cdiv(o.S, 16);
            return o;
        }
    } else {
        o.why = old_headmid_excluded(w, s, o.comp, S1);
    }
    int hv = 16;
    if (S2) {
        auto rounds = [&](int tf, long slots) { return old_rounds_of((long)cdiv(T, tf) * B, slots); };
        if (s.s2_head_tf)
            hv = s.s2_head_tf;
        else if ((long)cdiv(T, 16) * B >= 1024)
            hv = rounds(27, sl.head27) < rounds(24, sl.head24) ? 27 : 24;
        else
            hv = rounds(19, sl.head19) < rounds(16, sl.head16) ? 19 : 16;
    }
    if (S2 && o.comp && hv != 16) {
        if (hv == 19) o.head_tf = 19, o.head_waves = 8;
        else if (hv == 24) o.head_tf = 24, o.head_waves = 16;
        else o.head_tf = 27, o.head_waves = 16;
    } else {
        o.head_tf = S1 ? 63 : 16, o.head_waves = S1 ? 16 : 8;
    }
    if (w.mp) {  // launch_vocoder_midp
        int nch = s.midp_nch > 0 ? std::min(s.midp_nch, 4096) : 0;
        if (!nch) nch = old_strip(4 * T, B, 4, 256, 4);
        o.midp_nch = nch;
    }
    return o;
}

struct OldF32 {
    const char *head, *mid, *tail;
    bool pair, comp;
};
static OldF32 old_f32(const VocCall& c, const Switches& s) {
    const int plan = s.voc_plan, B = c.B, T = c.T;
    if (c.M == 64 && c.C == 128) {
        const int n16 = B * cdiv(T, 63), n8 = B * cdiv(T, 28);
        const double waste16 = (double)cdiv(n16, 256) * 256 / n16, waste8 = (double)cdiv(n8, 512) * 512 / n8;
        const bool w16 = plan == 2 || (plan < 0 && waste16 <= waste8);
        const bool pair = s.f32_pair && c.wt4p, comp = s.f32_comp && c.hcw;
        // s1_fused
        if (plan == 3) return {"S1W16s", "S1W16s", "S1W16s", pair, comp};
        if (w16) {
            switch (s.f32_mt) {
                case 1: return {"S1W16", "S1T8", "S1W16", pair, comp};
                case 2: return {"S1W16", "S1W16", "S1T8", pair, comp};
                case 3: return {"S1W16", "S1T8", "S1T8", pair, comp};
                case 4: return {"S1W16", "S1W16s", "S1T8", pair, comp};
                default: return {"S1W16", "S1W16", "S1W16", pair, comp};
            }
        }
        return {"S1W8", "S1W8", "S1W8", pair, comp};
    }
    if (c.M == 80 && c.C == 256) return {"S2W8", "S2W8", "S2W8", false, s.f32_comp && c.hcw};
    return {"TinyW8", "TinyW8", "TinyW8", false, false};
}

// grid.x windows of `width` cover [0, L) exactly once: the last one starts inside, none starts past the end
static bool covers(int gx, long width, long L) { return gx >= 1 && (gx - 1) * width < L && gx * width >= L; }

static VocCall voc_call_of(int stage, int B, int T) {
    VocCall c;
    c.M = stage == 1 ? 64 : 80, c.C = stage == 1 ? 128 : 256;
    c.B = B, c.T = T;
    c.hc = true, c.mp = stage == 1, c.tp = stage == 1, c.tp2 = stage == 2, c.redo_w = true;
    c.wt4p = stage == 1, c.hcw = true;
    c.fused = c.x3 = true;
    return c;
}

static const VocSlots kSlotsDefault{256, 256, 256, 256, 512, 512, 256, 256};  // MI355X, as the tilings' notes have it

static int g_plans = 0, g_plan_diff = 0, g_plan_inv = 0;

// One call: the plan against the old rules, and the plan's invariants.
static void check_plan(const VocCall& c, const Switches& s, const VocSlots& sl) {
    const VocLaunchPlan p = plan_vocoder_launch(c, s, sl);
    ++g_plans;
    const int B = c.B, T = c.T;
    bool same = true, inv = true;
    auto grid_ok = [&](const VocGrid& g) { return g.x >= 1 && g.y == B && g.threads >= 64 && g.lds >= 0 && g.lds <= 160 * 1024; };
    if (!c.x3) {
        const OldF32 o = old_f32(c, s);
        const f32::FormRow& f = f32::kF32Forms[p.form];
        const f32::Tiling &h = f32::kTiling[f.head], &m = f32::kTiling[f.mid], &t = f32::kTiling[f.tail];
        same = p.path == VocPath::F32 && !std::strcmp(h.name, o.head) && !std::strcmp(m.name, o.mid) &&
               !std::strcmp(t.name, o.tail) && p.pair == o.pair && p.f32_comp == o.comp && p.trans == c.trans &&
               p.redo == VocRedoPlan::None;
        inv = grid_ok(p.head_g) && grid_ok(p.mid_g) && grid_ok(p.tail_g) && covers(p.head_g.x, h.tf, T) &&
              covers(p.mid_g.x, m.w2, 4L * T) && covers(p.tail_g.x, t.w3, 16L * T) && p.head_g.threads == h.threads &&
              p.mid_g.threads == m.threads && p.tail_g.threads == t.threads;
    } else {
        const OldSplit o = old_split(c, s, sl);
        same = p.path == VocPath::Split && p.trans == c.trans && p.headmid == (o.n > 0) &&
               (p.no_headmid == nullptr) == (o.why == nullptr) &&
               (!o.why || !std::strcmp(p.no_headmid, o.why)) && p.comp == o.comp &&
               (int)p.redo == o.redo;
        if (p.headmid) {
            same = same && p.hm_n == o.n && p.hm_S == o.S && p.hm_nch == o.nch && p.head_g.x == o.n;
            inv = inv && grid_ok(p.head_g) && p.hm_S <= x3::kHeadmidSMax && p.hm_S >= 1 && covers(p.hm_n, p.hm_S, 4L * T) &&
                  16 * p.hm_nch >= p.hm_S && p.mid_g.threads == 0;
        } else {
            same = same && p.head_tf == o.head_tf && p.head_g.threads == o.head_waves * 64 &&
                   (p.mid == VocMid::Midp) == (o.midp_nch > 0) && p.mid_nch == o.midp_nch &&
                   (p.mid == VocMid::X3Alt) == o.alt_mid;
            inv = inv && grid_ok(p.head_g) && grid_ok(p.mid_g) && covers(p.head_g.x, p.head_tf, T) &&
                  covers(p.mid_g.x, p.mid == VocMid::Midp ? 16L * p.mid_nch : p.mid_w, 4L * T);
        }
        const bool tailp = p.tail == VocTail::Tailp || p.tail == VocTail::Tailp2;
        same = same && tailp == (o.tail_nl > 0) && p.tail_nl == o.tail_nl && p.tail_nch == o.tail_nch &&
               (p.tail == VocTail::Tailp2) == (c.tp2 && o.tail_nl > 0) && (p.tail == VocTail::X3Alt) == o.alt_tail;
        inv = inv && grid_ok(p.tail_g) && covers(p.tail_g.x, tailp ? 16L * p.tail_nch : p.tail_w, 16L * T);
        // exactly one redo strategy, and only the guarded one has a launch of its own
        const int strategies = (p.redo == VocRedoPlan::None) + (p.redo == VocRedoPlan::InTail) +
                               (p.redo == VocRedoPlan::Guarded) + (p.redo == VocRedoPlan::Host);
        inv = inv && strategies == 1 && (p.redo == VocRedoPlan::Guarded) == (p.redo_g.threads > 0) &&
              p.redo_g.lds <= 160 * 1024 && (p.redo != VocRedoPlan::InTail || tailp) &&
              ((c.range_policy == 1) == (p.redo != VocRedoPlan::None));
        if (p.redo == VocRedoPlan::Guarded) {
            const OldF32 of = old_f32(c, s);
            // RedoCfg: the 8-wave form of the stage
            const char* want = c.M == 64 ? "S1W8" : (c.M == 80 ? "S2W8" : "TinyW8");
            same = same && !std::strcmp(f32::kTiling[f32::kF32Forms[p.form].redo].name, want) && p.pair == of.pair &&
                   p.f32_comp == of.comp;
        }
    }
    char line[512];
    const int len = p.print(line, sizeof line);
    inv = inv && len > 0 && len < (int)sizeof line && (int)std::strlen(line) == len;
    if ((!same || !inv) && g_plan_diff + g_plan_inv < 5)
        std::printf("  stage %d B %d T %d: %s%s| %s\n", c.M == 64 ? 1 : 2, B, T, same ? "" : "DIFFERS ", inv ? "" : "INVARIANT ", line);
    g_plan_diff += !same;
    g_plan_inv += !inv;
}

static void expect_line(const char* what, const VocCall& c, const char* want) {
    char line[512];
    plan_vocoder_launch(c, Switches{}, kSlotsDefault).print(line, sizeof line);
    const bool ok = !std::strcmp(line, want);
    std::printf("  %s: %s%s\n", what, line, ok ? "" : " (UNEXPECTED)");
    g_bad += !ok;
}

static void check_launch_plans() {
    // the switch tables: the default, then each vocoder switch alone at each legal value and an illegal one
    std::vector<Switches> sws(1);
    auto with = [&](auto set) {
        Switches s;
        set(s);
        sws.push_back(s);
    };
    with([](Switches& s) { s.headmid = false; });
    for (const int v : {1, 5, 16, 4096, 5000, -3}) with([v](Switches& s) { s.midp_nch = v; });
    for (const int v : {8, 9, 21, 4096, 5000, -3}) with([v](Switches& s) { s.tailp_nch = v; });
    for (const int v : {8, 9, 4096, 5000, -3}) with([v](Switches& s) { s.tailp2_nch = v; });
    with([](Switches& s) { s.tailp_seven = true; });
    with([](Switches& s) { s.tailp2_seven = true; });
    with([](Switches& s) { s.head_inconv = true; });
    for (const int v : {0, 1, 2}) with([v](Switches& s) { s.s2_mid_alt = v; });
    for (const int v : {16, 19, 24, 27, 20}) with([v](Switches& s) { s.s2_head_tf = v; });
    for (const int v : {0, 2, 3, 7}) with([v](Switches& s) { s.voc_plan = v; });
    for (const int v : {0, 1, 2, 3, 4, 7}) with([v](Switches& s) { s.f32_mt = v; });
    with([](Switches& s) { s.f32_pair = false; });
    with([](Switches& s) { s.f32_comp = false; });
    with([](Switches& s) { s.redo_launch = true; });
    // the slot counts: the default, each count alone at 256 / 512 / 768, all of them at each, and 304 CUs
    std::vector<VocSlots> slots(1, kSlotsDefault);
    for (const long v : {256L, 512L, 768L}) {
        for (int f = 0; f < 8; ++f) {
            VocSlots sl = kSlotsDefault;
            (&sl.head16)[f] = v;
            slots.push_back(sl);
        }
        slots.push_back({v, v, v, v, v, v, v, v});
    }
    slots.push_back({304, 304, 304, 304, 608, 608, 304, 304});
    std::vector<int> Ts;
    for (int t = 1; t <= 300; ++t) Ts.push_back(t);
    Ts.push_back(500), Ts.push_back(2600);
    // the handles: every pack, the x3 mid / tail kept (M2_VOC_MID_X3 / M2_VOC_TAIL_X3), no composed head,
    // the exact-f32 path with and without its stage1 packs; the range policies
    struct Handle {
        bool mp, tail, hc, x3, f32_packs;
    };
    const Handle handles[] = {{true, true, true, true, true},   {false, true, true, true, true},
                              {true, false, true, true, true},  {false, false, true, true, true},
                              {true, true, false, true, true},  {true, true, true, false, true},
                              {true, true, true, false, false}};
    struct Policy {
        int policy, redo;
    };
    const Policy policies[] = {{0, -1}, {1, -1}, {1, 0}, {1, 1}};
    for (int stage = 1; stage <= 2; ++stage)
        for (const int B : {1, 2, 3, 8, 16, 32, 64, 128})
            for (const int T : Ts) {
                const VocCall base = voc_call_of(stage, B, T);
                // calls x (switch tables with the default slots, slot counts with the default switches)
                for (int layout = 0; layout < 2; ++layout)
                    for (int dev = 0; dev < 2; ++dev)
                        for (const unsigned prof : {0u, 1u, 2u, 4u}) {
                            VocCall c = base;
                            c.trans = layout, c.device_T = dev, c.prof_slots = prof;
                            for (const Switches& s : sws) check_plan(c, s, kSlotsDefault);
                            for (size_t i = 1; i < slots.size(); ++i) check_plan(c, sws[0], slots[i]);
                        }
                // handles x policies x switch tables
                for (const Handle& h : handles)
                    for (const Policy& pol : policies) {
                        VocCall c = base;
                        c.mp = c.mp && h.mp, c.tp = c.tp && h.tail, c.tp2 = c.tp2 && h.tail, c.hc = h.hc;
                        c.redo_w = c.tp || c.tp2;
                        c.x3 = h.x3, c.wt4p = c.wt4p && h.f32_packs, c.hcw = h.f32_packs;
                        c.range_policy = pol.policy, c.redo = h.x3 ? pol.redo : -1;
                        for (const Switches& s : sws) check_plan(c, s, kSlotsDefault);
                        check_plan(c, sws[0], slots.back());
                    }
            }
    {  // the tiny shape (exact-f32 only) and a handle without the fused kernels
        VocCall c = voc_call_of(1, 2, 40);
        c.M = 32, c.C = 64, c.x3 = c.hc = c.mp = c.tp = c.redo_w = c.wt4p = c.hcw = false;
        check_plan(c, sws[0], kSlotsDefault);
        c.fused = false;
        char line[64];
        plan_vocoder_launch(c, sws[0], kSlotsDefault).print(line, sizeof line);
        g_plan_diff += std::strcmp(line, "perlayer") != 0;
    }
    std::printf("launch plans: %d plans over %zu switch tables and %zu slot sets, %d differ from the old rules, %d break "
                "an invariant\n",
                g_plans, sws.size(), slots.size(), g_plan_diff, g_plan_inv);
    g_bad += g_plan_diff + g_plan_inv;
    // the headline and the two stage2 bench lines, literally ([B, M, T] mel, host T, default switches)
    expect_line("stage1 B=32 T=500", voc_call_of(1, 32, 500), "split stage=1 headmid[n=8 S=250 nch=16 trans=0 grid=8x32 thr=1024 lds=148608] "
                "tailp[nl=6 nch=21 grid=24x32 thr=448 lds=49184] redo=none");
    expect_line("stage2 B=8 T=500", voc_call_of(2, 8, 500), "split stage=2 head[tf=16 comp=1 trans=0 grid=32x8 thr=512 lds=81600] "
                "x3mid[alt=1 w=33 grid=61x8 thr=512 lds=81216] tailp2[nl=6 nch=16 grid=32x8 thr=768 lds=98352] redo=none "
                "no-headmid=\"not the stage1 shapes\"");
    expect_line("stage2 B=16 T=2600", voc_call_of(2, 16, 2600), "split stage=2 head[tf=24 comp=1 trans=0 grid=109x16 thr=1024 lds=116416] "
                "x3mid[alt=0 w=30 grid=347x16 thr=512 lds=73152] tailp2[nl=6 nch=163 grid=16x16 thr=768 lds=98352] "
                "redo=none no-headmid=\"not the stage1 shapes\"");
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

// carve_spectral_bwd: one buffer of n_fft floats per frame, 1 + L / hop frames per utterance.  The
// Sizer's count is that product, a Carve over exactly that many bytes places the buffer at the
// base and one byte fewer is refused; at hop n_fft / 4 it is 16 bytes per sample and frame 0's share.
static void check_spectral_bwd() {
    int bad = 0, carved = 0;
    for (const int n_fft : {512, 1024, 2048})
        for (const int hop : {n_fft / 4, 200, 1})
            for (const int B : {1, 2, 32})
                for (const int L : {n_fft / 2 + 1, 777, 2624, 32000}) {
                    if (L <= n_fft / 2) continue;
                    const int frames = loss::spectral_frames(L, hop);
                    const size_t want = (size_t)B * frames * n_fft * sizeof(float);
                    Sizer s;
                    loss::carve_spectral_bwd(s, n_fft, hop, B, L, nullptr);
                    bad += frames != 1 + L / hop || s.off != want;
                    if (hop == n_fft / 4) bad += want != (size_t)B * (16 * (size_t)(L / hop) * hop + 4 * n_fft);
                    if (want > ((size_t)64 << 20)) continue;
                    ++carved;
                    std::vector<char> mem(want);
                    Carve c(mem.data(), mem.size()), less(mem.data(), mem.size() - 1);
                    float *fr = nullptr, *none = nullptr;
                    loss::carve_spectral_bwd(c, n_fft, hop, B, L, &fr);
                    loss::carve_spectral_bwd(less, n_fft, hop, B, L, &none);
                    bad += !c.ok || less.ok || reinterpret_cast<char*>(fr) != mem.data() || none != nullptr;
                }
    std::printf("spectral_bwd:");
    expect("carve_exact", bad == 0 && carved > 0, true);
    std::printf(" (%d carved)\n", carved);
}

// The vocoder's gradient plan over C x T x B.  Restated plainly: the tape is h [C, T], three maps
// [C / 2^(k+1), T x 4, 16, 32, 64] per stage and the audio [1, 64 T], B of each, every map on a 256-byte
// boundary; the workspace is three buffers of B x the widest map, the partials of the widest
// reduction, and one weight and one bias of the largest size.  A Carve over exactly the Sizer's bytes succeeds and one byte fewer is refused; the
// carved regions are in order and disjoint; every row fits 48 KiB of LDS and the grid limits.
static void check_vocoder_grad() {
    int bad = 0, plans = 0, rows_seen = 0, narrow = 0;
    const int rates[4] = {4, 4, 2, 2};
    for (const int C : {16, 32, 128, 256})
        for (const int T : {1, 17, 70, 500})
            for (const int B : {1, 3, 32}) {
                const vgrad::Dims d{C == 256 ? 80 : C == 32 ? 5 : 64, C, B, T};
                bad += !vgrad::dims_ok(d);
                ++plans;
                // the tape
                size_t off = 0, widest = (size_t)C * T;
                std::vector<size_t> at, len;
                auto put = [&](size_t floats) {
                    off = (off + 255) / 256 * 256;
                    at.push_back(off);
                    len.push_back(floats * 4);
                    off += floats * 4;
                };
                put((size_t)B * C * T);
                int L = T;
                for (int k = 0; k < 4; ++k) {
                    L *= rates[k];
                    const size_t n = (size_t)(C >> (k + 1)) * L;
                    widest = std::max(widest, n);
                    for (int j = 0; j < 3; ++j) put((size_t)B * n);
                }
                put((size_t)B * 64 * T);
                Sizer ts;
                vgrad::carve_tape(ts, d, nullptr);
                bad += ts.off != off || at.size() != (size_t)vgrad::kMaps;
                std::vector<char> mem(off);
                Carve tc(mem.data(), mem.size()), less(mem.data(), mem.size() - 1);
                float *maps[vgrad::kMaps], *none[vgrad::kMaps];
                vgrad::carve_tape(tc, d, maps);
                vgrad::carve_tape(less, d, none);
                bad += !tc.ok || less.ok;
                for (int i = 0; i < vgrad::kMaps && tc.ok; ++i) {
                    bad += reinterpret_cast<char*>(maps[i]) != mem.data() + at[i];
                    if (i > 0) bad += at[i] < at[i - 1] + len[i - 1];  // no overlap
                    int c, n;
                    vgrad::map_shape(d, i, &c, &n);
                    bad += (size_t)B * c * n * 4 != len[i];
                }
                // the workspace
                size_t part = (size_t)B * ((64 * T + 1023) / 1024) * (3 * (size_t)(C >> 4) + 1);
                for (const vgrad::Step& s : vgrad::plan_steps(d)) {
                    if (s.kind != vgrad::STEP_WGRAD && s.kind != vgrad::STEP_IN) continue;
                    const size_t n = (size_t)s.g.Cout * s.g.Cin * s.g.k;
                    const int Lo = loss::conv_out_len(s.L, s.g);
                    size_t want;
                    if (s.g.Cout < 16) {
                        const long long chunks = (long long)B * ((Lo + 255) / 256);
                        const long long cps = (chunks + std::min<long long>(chunks, 512) - 1) / std::min<long long>(chunks, 512);
                        want = (size_t)((chunks + cps - 1) / cps) * (n + s.g.Cout);
                        bad += !s.narrow;
                        ++narrow;
                    } else {
                        const long long chunks = (long long)B * ((Lo + 63) / 64);
                        want = (size_t)std::max<long long>(1, std::min<long long>({chunks, 64, (long long)(1 + (8u << 20) / n)})) * n;
                        bad += s.narrow || !loss::dw_plan(s.g, B, s.L).mfma;
                    }
                    bad += vgrad::step_part_floats(s, B) != want;
                    part = std::max(part, want);
                }
                bad += vgrad::part_floats(d) != part || vgrad::widest_map(d) != widest;
                size_t woff = 0;
                const size_t weight = std::max((size_t)3 * C * d.M, (size_t)4 * C * C);  // the input conv, or ConvT_0
                bad += vgrad::widest_weight(d) != weight || vgrad::widest_bias(d) != (size_t)C;
                for (const size_t floats : {B * widest, B * widest, B * widest, part, weight, (size_t)C}) woff = (woff + 255) / 256 * 256 + floats * 4;
                Sizer ws;
                vgrad::carve_backward(ws, d, nullptr);
                bad += ws.off != woff;
                if (woff <= ((size_t)160 << 20)) {
                    std::vector<char> wm(woff);
                    Carve wc(wm.data(), wm.size()), wless(wm.data(), wm.size() - 1);
                    vgrad::Bufs b{}, nb{};
                    vgrad::carve_backward(wc, d, &b);
                    vgrad::carve_backward(wless, d, &nb);
                    bad += !wc.ok || wless.ok;
                    const char* p[7] = {reinterpret_cast<char*>(b.cot[0]), reinterpret_cast<char*>(b.cot[1]),
                                        reinterpret_cast<char*>(b.gv), reinterpret_cast<char*>(b.part),
                                        reinterpret_cast<char*>(b.wtmp), reinterpret_cast<char*>(b.btmp),
                                        wm.data() + wm.size()};
                    const size_t bytes[6] = {B * widest * 4, B * widest * 4, B * widest * 4, part * 4, weight * 4,
                                             (size_t)C * 4};
                    bad += p[0] != wm.data();
                    for (int i = 0; i < 5; ++i) bad += p[i + 1] < p[i] + bytes[i];  // no overlap
                    bad += p[6] != p[5] + bytes[5];
                }
                // the rows
                for (const vgrad::Step& s : vgrad::plan_steps(d)) {
                    std::vector<loss::LaunchRow> rows;
                    vgrad::step_rows(s, B, true, s.dw >= 0, s.db >= 0, rows);
                    bad += rows.empty();
                    for (const loss::LaunchRow& r : rows) {
                        ++rows_seen;
                        bad += r.lds > (size_t)loss::kMaxLds || r.gx < 1 || r.gy < 1 || r.gz < 1 || r.gy > 65535 ||
                               r.gz > 65535 || (r.threads != 256 && r.threads != loss::kDbThreads);
                        if (C >= 128 && B * T >= 500)
                            bad += !std::strcmp(r.kernel, "conv_dw_direct_kernel") ||
                                   !std::strcmp(r.kernel, "conv_dx_direct_kernel");
                    }
                }
                bad += vgrad::print_plan(d).find("out:voc_out_bwd_kernel[grid=") == std::string::npos;
            }
    for (const int c : {1, 2, 8, 16, 64, 128}) bad += vgrad::res_width(c) < 32 || vgrad::res_lds_bytes(c) > (size_t)loss::kMaxLds;
    bad += vgrad::dims_ok(vgrad::Dims{64, 120, 1, 4}) || vgrad::dims_ok(vgrad::Dims{64, 512, 1, 4}) ||
           vgrad::dims_ok(vgrad::Dims{0, 128, 1, 4});
    std::printf("vocoder_grad:");
    expect("plans_match", bad == 0 && plans == 48 && narrow > 0, true);
    std::printf(" (%d plans, %d rows)\n", plans, rows_seen);
}

// The decoder's gradient plan (csrc/decoder_grad_plan.h) over the stage1 and stage2 training shapes and a
// few small ones.  Restated plainly: the tape is five maps [R, 3H | H | H | 2H | H] per layer, each on a
// 256-byte boundary; the workspace is two maps [R, H], one [R, 3H], the statistics [B, heads, T, 3] and
// the partials of the widest reduction.  A Carve over exactly the Sizer's bytes succeeds and one byte
// fewer is refused; the carved regions are in order and disjoint; every row fits 48 KiB of LDS and the
// grid limits; every weight gradient's partials fit `part`.
static void check_decoder_grad() {
    int bad = 0, plans = 0, rows_seen = 0;
    const int shapes[][6] = {{64, 64, 2, 2, 32, 500}, {96, 80, 3, 2, 8, 500}, {32, 5, 1, 2, 3, 1},
                             {128, 80, 1, 2, 1, 65},  {64, 64, 1, 4, 2, 33},  {64, 64, 2, 2, 1, 1}};
    for (const auto& sh : shapes) {
        const dgrad::Dims d{sh[0], sh[1], sh[2], sh[3], sh[4], sh[5]};
        bad += !dgrad::dims_ok(d);
        ++plans;
        const size_t R = (size_t)d.B * d.T, H = (size_t)d.H;
        // the tape
        size_t off = 0;
        std::vector<size_t> at, len;
        auto put = [&](size_t floats) {
            off = (off + 255) / 256 * 256;
            at.push_back(off);
            len.push_back(floats * 4);
            off += floats * 4;
        };
        for (int l = 0; l < d.layers; ++l)
            for (const size_t w : {3 * H, H, H, 2 * H, H}) put(R * w);
        Sizer ts;
        dgrad::carve_tape(ts, d, nullptr);
        bad += ts.off != off || at.size() != (size_t)dgrad::n_maps(d);
        std::vector<char> mem(off);
        Carve tc(mem.data(), mem.size()), less(mem.data(), mem.size() - 1);
        std::vector<float*> maps(at.size()), none(at.size());
        dgrad::carve_tape(tc, d, maps.data());
        dgrad::carve_tape(less, d, none.data());
        bad += !tc.ok || less.ok;
        for (size_t i = 0; i < at.size() && tc.ok; ++i) {
            bad += reinterpret_cast<char*>(maps[i]) != mem.data() + at[i];
            if (i > 0) bad += at[i] < at[i - 1] + len[i - 1];  // no overlap
            bad += R * dgrad::map_width(d, (int)i) * 4 != len[i];
        }
        // the workspace
        size_t part = (R + 63) / 64 * 2 * H;
        for (const dgrad::Step& s : dgrad::plan_steps(d)) {
            if (s.kind != dgrad::STEP_DW) continue;
            const long long tiles = (s.N + 63) / 64, chunks = (long long)((R + 31) / 32);
            const long long want = std::max<long long>(1, std::min<long long>(chunks, (256 + tiles - 1) / tiles));
            const long long rps = (chunks + want - 1) / want * 32, splits = ((long long)R + rps - 1) / rps;
            const size_t need = (size_t)splits * ((size_t)s.N * s.K + s.N);
            bad += dgrad::step_part_floats(s, d) != need || splits < 1 || splits > 256 || rps * splits < (long long)R;
            part = std::max(part, need);
        }
        bad += dgrad::part_floats(d) != part;
        size_t woff = 0;
        const size_t floats[5] = {R * H, R * H, R * 3 * H, (size_t)d.B * d.heads * d.T * 3, part};
        for (const size_t f : floats) woff = (woff + 255) / 256 * 256 + f * 4;
        Sizer ws;
        dgrad::carve_backward(ws, d, nullptr);
        bad += ws.off != woff;
        {
            std::vector<char> wm(woff);
            Carve wc(wm.data(), wm.size()), wless(wm.data(), wm.size() - 1);
            dgrad::Bufs b{}, nb{};
            dgrad::carve_backward(wc, d, &b);
            dgrad::carve_backward(wless, d, &nb);
            bad += !wc.ok || wless.ok;
            const char* p[6] = {reinterpret_cast<char*>(b.cot[0]), reinterpret_cast<char*>(b.cot[1]),
                                reinterpret_cast<char*>(b.wide),   reinterpret_cast<char*>(b.stats),
                                reinterpret_cast<char*>(b.part),   wm.data() + wm.size()};
            bad += p[0] != wm.data();
            for (int i = 0; i < 4; ++i) bad += p[i + 1] < p[i] + floats[i] * 4;  // no overlap
            bad += p[5] != p[4] + floats[4] * 4;
        }
        // the rows
        int steps = 0;
        for (const dgrad::Step& s : dgrad::plan_steps(d)) {
            ++steps;
            std::vector<loss::LaunchRow> rows;
            const bool ln = s.kind == dgrad::STEP_DX && s.mode == dgrad::DX_LN;
            dgrad::step_rows(s, d, true, s.kind == dgrad::STEP_DW ? s.dw >= 0 : ln,
                             s.kind == dgrad::STEP_DW ? s.db >= 0 : ln, rows);
            bad += rows.empty();
            if (s.kind == dgrad::STEP_DX) bad += !dgrad::dx_ok(s.K, s.N, s.mode);
            if (s.kind == dgrad::STEP_DW) bad += !dgrad::dw_ok(s.K, s.N);
            for (const loss::LaunchRow& r : rows) {
                ++rows_seen;
                bad += r.lds > (size_t)loss::kMaxLds || r.gx < 1 || r.gy < 1 || r.gz < 1 || r.gy > 65535 ||
                       r.gz > 65535 || r.threads != 256;
            }
        }
        bad += steps != 2 + 9 * d.layers;
        bad += dgrad::print_plan(d).find(" mw:lin_dw_kernel[grid=") == std::string::npos;
    }
    bad += dgrad::dims_ok(dgrad::Dims{60, 64, 2, 2, 1, 4}) || dgrad::dims_ok(dgrad::Dims{160, 64, 2, 4, 1, 4}) ||
           dgrad::dims_ok(dgrad::Dims{64, 64, 2, 8, 1, 4}) || dgrad::dims_ok(dgrad::Dims{64, 0, 2, 2, 1, 4}) ||
           dgrad::dims_ok(dgrad::Dims{64, 64, 0, 2, 1, 4});
    std::printf("decoder_grad:");
    expect("plans_match", bad == 0 && plans == 6, true);
    std::printf(" (%d plans, %d rows)\n", plans, rows_seen);
}

// The text encoder's gradient plan (csrc/encoder_grad_plan.h) over the stage1 and stage2 training shapes
// and the test cases.  Restated plainly: the tape is x0 [R, H] and then the decoder's five maps per layer;
// the workspace is the decoder's, its partials the widest of the final norm's slots, the layers' weight
// gradients and the embedding's [splits][V][H]; a vocabulary row's positions are split into whole
// 64-position chunks, about 256 workgroups in all.  Sizes, overlaps and launch limits as check_decoder_grad.
static void check_encoder_grad() {
    int bad = 0, plans = 0, rows_seen = 0;
    const int shapes[][6] = {{256, 64, 2, 2, 32, 100}, {256, 96, 3, 2, 8, 100}, {256, 64, 2, 2, 2, 7},
                             {256, 96, 3, 2, 1, 5},    {5, 32, 1, 2, 3, 1},     {40, 64, 2, 2, 2, 130},
                             {300, 96, 1, 2, 1, 67},   {256, 128, 1, 2, 1, 65}, {256, 64, 1, 4, 3, 33}};
    for (const auto& sh : shapes) {
        const egrad::Dims d{sh[0], sh[1], sh[2], sh[3], sh[4], sh[5]};
        bad += !egrad::dims_ok(d);
        ++plans;
        const size_t R = (size_t)d.B * d.S, H = (size_t)d.H, V = (size_t)d.V;
        // the tape
        size_t off = 0;
        std::vector<size_t> at, len;
        auto put = [&](size_t floats) {
            off = (off + 255) / 256 * 256;
            at.push_back(off);
            len.push_back(floats * 4);
            off += floats * 4;
        };
        put(R * H);
        for (int l = 0; l < d.layers; ++l)
            for (const size_t w : {3 * H, H, H, 2 * H, H}) put(R * w);
        Sizer ts;
        egrad::carve_tape(ts, d, nullptr);
        bad += ts.off != off || at.size() != (size_t)egrad::n_maps(d);
        std::vector<char> mem(off);
        Carve tc(mem.data(), mem.size()), less(mem.data(), mem.size() - 1);
        std::vector<float*> maps(at.size()), none(at.size());
        egrad::carve_tape(tc, d, maps.data());
        egrad::carve_tape(less, d, none.data());
        bad += !tc.ok || less.ok;
        for (size_t i = 0; i < at.size() && tc.ok; ++i) {
            bad += reinterpret_cast<char*>(maps[i]) != mem.data() + at[i];
            if (i > 0) bad += at[i] < at[i - 1] + len[i - 1];  // no overlap
            bad += R * egrad::map_width(d, (int)i) * 4 != len[i];
        }
        // the embedding's split and the workspace
        const long long chunks = (long long)((R + 63) / 64);
        const long long want = std::max<long long>(1, std::min<long long>(chunks, (256 + (long long)V - 1) / (long long)V));
        const long long rps = (chunks + want - 1) / want * 64, splits = ((long long)R + rps - 1) / rps;
        const egrad::EmbPlan ep = egrad::emb_split(R, d.V, d.H);
        bad += ep.rps != rps || ep.splits != splits || ep.part_floats != (size_t)splits * V * H || splits < 1 ||
               rps * splits < (long long)R || (V >= 256 && splits != 1) || (long long)V * splits > 256 + (long long)V;
        size_t part = std::max((R + 63) / 64 * 2 * H, ep.part_floats);
        for (const dgrad::Step& s : egrad::plan_steps(d)) {
            if (s.kind != dgrad::STEP_DW) continue;
            const size_t need = dgrad::dw_split(R, s.K, s.N).part_floats;  // check_decoder_grad restates it
            bad += egrad::step_part_floats(s, d) != need;
            part = std::max(part, need);
        }
        bad += egrad::part_floats(d) != part;
        size_t woff = 0;
        const size_t floats[5] = {R * H, R * H, R * 3 * H, (size_t)d.B * d.heads * d.S * 3, part};
        for (const size_t f : floats) woff = (woff + 255) / 256 * 256 + f * 4;
        Sizer ws;
        egrad::carve_backward(ws, d, nullptr);
        bad += ws.off != woff;
        {
            std::vector<char> wm(woff);
            Carve wc(wm.data(), wm.size()), wless(wm.data(), wm.size() - 1);
            dgrad::Bufs b{}, nb{};
            egrad::carve_backward(wc, d, &b);
            egrad::carve_backward(wless, d, &nb);
            bad += !wc.ok || wless.ok;
            const char* p[6] = {reinterpret_cast<char*>(b.cot[0]), reinterpret_cast<char*>(b.cot[1]),
                                reinterpret_cast<char*>(b.wide),   reinterpret_cast<char*>(b.stats),
                                reinterpret_cast<char*>(b.part),   wm.data() + wm.size()};
            bad += p[0] != wm.data();
            for (int i = 0; i < 4; ++i) bad += p[i + 1] < p[i] + floats[i] * 4;  // no overlap
            bad += p[5] != p[4] + floats[4] * 4;
        }
        // the rows
        int steps = 0;
        const std::vector<dgrad::Step> plan = egrad::plan_steps(d);
        for (const dgrad::Step& s : plan) {
            ++steps;
            std::vector<loss::LaunchRow> rows;
            const bool ln = s.kind == dgrad::STEP_LN || (s.kind == dgrad::STEP_DX && s.mode == dgrad::DX_LN);
            const bool w = s.kind == dgrad::STEP_DW || s.kind == dgrad::STEP_EMB;
            egrad::step_rows(s, d, true, w ? s.dw >= 0 : ln, w ? s.db >= 0 : ln, rows);
            bad += rows.empty();
            if (s.kind == dgrad::STEP_DX) bad += !dgrad::dx_ok(s.K, s.N, s.mode);
            if (s.kind == dgrad::STEP_DW) bad += !dgrad::dw_ok(s.K, s.N);
            if (s.kind == dgrad::STEP_LN) bad += !egrad::ln_ok(s.K);
            if (s.kind == dgrad::STEP_EMB) bad += !egrad::emb_ok(d.V, d.H);
            for (const loss::LaunchRow& r : rows) {
                ++rows_seen;
                bad += r.lds > (size_t)loss::kMaxLds || r.gx < 1 || r.gy < 1 || r.gz < 1 || r.gy > 65535 ||
                       r.gz > 65535 || r.threads != 256;
            }
        }
        bad += steps != 2 + 9 * d.layers || plan.front().kind != dgrad::STEP_LN || plan.back().kind != dgrad::STEP_EMB;
        // layer 0's qx reads x0 and writes the cotangent the embedding reads
        const dgrad::Step& qx0 = plan[plan.size() - 2];
        bad += qx0.aux != 0 || qx0.out != dgrad::BUF_DX || plan.back().gy != dgrad::BUF_DX || plan.back().dw != 0;
        const std::string line = egrad::print_plan(d);
        bad += line.find(" nx:ln_bwd_kernel[grid=") == std::string::npos ||
               line.find(" ew:emb_dw_kernel[grid=") == std::string::npos;
        const loss::LaunchRow lr = egrad::lr_row(d.B, d.S);
        bad += lr.gx != (unsigned)((d.S + 3) / 4) || lr.gy != (unsigned)d.B || lr.threads != 256 || lr.lds != 0;
    }
    bad += egrad::dims_ok(egrad::Dims{0, 64, 2, 2, 1, 4}) || egrad::dims_ok(egrad::Dims{65537, 64, 2, 2, 1, 4}) ||
           egrad::dims_ok(egrad::Dims{256, 60, 2, 2, 1, 4}) || egrad::dims_ok(egrad::Dims{256, 160, 2, 4, 1, 4}) ||
           egrad::dims_ok(egrad::Dims{256, 64, 2, 8, 1, 4}) || egrad::dims_ok(egrad::Dims{256, 64, 0, 2, 1, 4});
    bad += !egrad::dims_ok(egrad::Dims{65536, 128, 1, 2, 1, 4}) || !egrad::dims_ok(egrad::Dims{1, 64, 1, 2, 1, 4});
    std::printf("encoder_grad:");
    expect("plans_match", bad == 0 && plans == 9, true);
    std::printf(" (%d plans, %d rows)\n", plans, rows_seen);
}

// The duration predictor's gradient plan (csrc/duration_grad_plan.h) over the stage1 training shape and
// the test cases.  Restated plainly: the tape is y1 and y2 [B, H, S]; the workspace is four maps of that
// size (xt, u, gu, gy), the partials (the wider of the head's slots, one of 3 H + 1 floats per utterance
// and 64-position chunk, and the conv weight gradient's split partials), one conv weight [H, H, 3] and one
// bias [H]; eight steps, the first and last the transposes.  Sizes, overlaps and launch limits as
// check_decoder_grad.
static void check_duration_grad() {
    int bad = 0, plans = 0, rows_seen = 0;
    const int shapes[][3] = {{64, 32, 100}, {64, 2, 100}, {32, 1, 1},  {32, 3, 63}, {96, 2, 64},
                             {128, 2, 65},  {64, 1, 130}, {16, 2, 7},  {24, 2, 33}};
    for (const auto& sh : shapes) {
        const dugrad::Dims d{sh[0], sh[1], sh[2]};
        bad += !dugrad::dims_ok(d);
        ++plans;
        const size_t H = (size_t)d.H, B = (size_t)d.B, S = (size_t)d.S, n = B * H * S;
        // the tape
        const size_t second = (n * 4 + 255) / 256 * 256, tape = second + n * 4;
        Sizer ts;
        dugrad::carve_tape(ts, d, nullptr);
        bad += ts.off != tape;
        {
            std::vector<char> mem(tape);
            Carve tc(mem.data(), mem.size()), less(mem.data(), mem.size() - 1);
            float *maps[dugrad::kMaps], *none[dugrad::kMaps];
            dugrad::carve_tape(tc, d, maps);
            dugrad::carve_tape(less, d, none);
            bad += !tc.ok || less.ok;
            if (tc.ok)
                bad += reinterpret_cast<char*>(maps[0]) != mem.data() || reinterpret_cast<char*>(maps[1]) != mem.data() + second;
        }
        // the partials and the workspace
        const size_t nslots = B * ((S + 63) / 64);
        const size_t part = std::max(nslots * (3 * H + 1), loss::dw_plan(loss::ConvGeo{d.H, d.H, 3, 1, 1, 1}, d.B, d.S).part_floats);
        bad += dugrad::part_floats(d) != part || dugrad::slots(d) != nslots || dugrad::slot_floats(d.H, false) != 2 * H;
        const size_t floats[7] = {n, n, n, n, part, 3 * H * H, H};
        size_t woff = 0;
        for (const size_t f : floats) woff = (woff + 255) / 256 * 256 + f * 4;
        Sizer ws;
        dugrad::carve_backward(ws, d, nullptr);
        bad += ws.off != woff;
        {
            std::vector<char> wm(woff);
            Carve wc(wm.data(), wm.size()), wless(wm.data(), wm.size() - 1);
            dugrad::Bufs b{}, nb{};
            dugrad::carve_backward(wc, d, &b);
            dugrad::carve_backward(wless, d, &nb);
            bad += !wc.ok || wless.ok;
            const char* p[8] = {reinterpret_cast<char*>(b.xt),   reinterpret_cast<char*>(b.u),    reinterpret_cast<char*>(b.gu),
                                reinterpret_cast<char*>(b.gy),   reinterpret_cast<char*>(b.part), reinterpret_cast<char*>(b.wtmp),
                                reinterpret_cast<char*>(b.btmp), wm.data() + wm.size()};
            bad += p[0] != wm.data();
            for (int i = 0; i < 6; ++i) bad += p[i + 1] < p[i] + floats[i] * 4;  // no overlap
            bad += p[7] != p[6] + floats[6] * 4;
        }
        // the rows
        const std::vector<dugrad::Step> plan = dugrad::plan_steps(d);
        bad += plan.size() != 8 || plan.front().kind != dugrad::STEP_XT || plan.back().kind != dugrad::STEP_DT;
        int finishes = 0, convs = 0;
        for (const dugrad::Step& s : plan) {
            std::vector<loss::LaunchRow> rows, rows_acc;
            dugrad::step_rows(s, d, false, rows);
            dugrad::step_rows(s, d, true, rows_acc);
            bad += rows.empty() || rows_acc.size() != rows.size() + (s.kind == dugrad::STEP_CONV ? 2 : 0);
            for (const loss::LaunchRow& r : rows_acc) {
                ++rows_seen;
                const bool db = std::strcmp(r.kernel, "conv_db_kernel") == 0;
                bad += r.lds > (size_t)loss::kMaxLds || r.gx < 1 || r.gy < 1 || r.gz < 1 || r.gy > 65535 ||
                       r.gz > 65535 || r.threads != (db ? loss::kDbThreads : 256);
                finishes += std::strcmp(r.kernel, "dec_finish_kernel") == 0;
                convs += std::strcmp(r.kernel, "conv_dx_mfma_kernel") == 0 || std::strcmp(r.kernel, "conv_dw_mfma_kernel") == 0;
            }
        }
        bad += finishes != 10 || convs != 4;  // both convs take the exact-f32 MFMA for the data and the weight gradient
        const loss::LaunchRow hd = dugrad::bn_row(d, true), b1 = dugrad::bn_row(d, false);
        bad += hd.gx != (unsigned)((S + 63) / 64) || hd.gy != (unsigned)B || hd.lds != H * 64 * 4 || b1.lds != 0 ||
               b1.gx != hd.gx;
        const loss::LaunchRow xt = dugrad::tr_row(d.B, d.S, d.H), cf = dugrad::conv_fwd_row(d);
        bad += xt.gx != (unsigned)((H + 31) / 32) || xt.gy != (unsigned)((S + 31) / 32) || xt.gz != (unsigned)B;
        bad += cf.gx != (unsigned)((S + 1023) / 1024) || cf.gy != (unsigned)(H / 8) || cf.gz != (unsigned)B;
        const std::string line = dugrad::print_plan(d);
        char head[128];
        std::snprintf(head, sizeof(head), "H=%d B=%d S=%d tape=%zu ws=%zu part=%zu u=recomputed xt:dur_transpose_kernel[grid=",
                      d.H, d.B, d.S, tape + 256, woff + 256, part);
        bad += line.compare(0, std::strlen(head), head) != 0 ||
               line.find(" hd:dur_bn_bwd_kernel[grid=") == std::string::npos ||
               line.find(" c1:conv_dw_mfma_kernel[grid=") == std::string::npos ||
               line.find(" dt:dur_transpose_kernel[grid=") == std::string::npos;
    }
    bad += dugrad::dims_ok(dugrad::Dims{8, 1, 4}) || dugrad::dims_ok(dugrad::Dims{60, 1, 4}) ||
           dugrad::dims_ok(dugrad::Dims{136, 1, 4}) || dugrad::dims_ok(dugrad::Dims{64, -1, 4}) ||
           dugrad::dims_ok(dugrad::Dims{64, 1, (1 << 20) + 1});
    bad += dugrad::dims_ok(dugrad::Dims{128, 16, 1 << 20});  // a map above 2^30 floats
    bad += !dugrad::dims_ok(dugrad::Dims{16, 0, 0}) || !dugrad::dims_ok(dugrad::Dims{128, 8, 1 << 20});
    std::printf("duration_grad:");
    expect("plans_match", bad == 0 && plans == 9, true);
    std::printf(" (%d plans, %d rows)\n", plans, rows_seen);
}

// ---------------------------------------------------------------------------
// The transformer stacks' launch plan (csrc/transformer_plan.h) against the rules the drivers
// and launchers carried before it: tfl_use / tf_chain / tf_first_fused / text_encoder_layers /
// mel_decoder / run_tfl / run_stack / run_layer / final_projection of m2_runtime.hip, tfl_rb /
// tfl_qs2 and the launchers' own overrides of transformer_layer.hip, tf_waves of
// transformer_fused.hip.  Each old_* returns the launch sequence with its geometry.
struct OldTfCall {
    int H, heads, n, mel;  // mel 0: the encoder's call (no final projection)
    bool tfused, att_f32, wide_last;
    int src;  // 0 x, 1 embed, 2 expand
    bool masked, devT, ragged;
    int B, N;
};
struct OldTfRow {
    const char* kind;
    int layer, next, op, rb, qs2, waves, grid, thr;
};
struct OldTf {
    int form = 0;
    int32_t err = 0;
    const char* msg = nullptr;
    bool projected = false;
    std::vector<OldTfRow> rows;
};
static bool old_tfl_supported(int H, int heads) { return heads == 2 && (H == 32 || H == 64 || H == 96); }
static bool old_tfl_proj_supported(int H, int NN) {
    return (H == 32 && (NN == 32 || NN == 64)) || (H == 64 && (NN == 64 || NN == 80)) || (H == 96 && (NN == 80 || NN == 96));
}
static bool old_post_next_supported(int H, int NN) {
    return (H == 32 && (NN == 96 || NN == 32 || NN == 64)) || (H == 64 && (NN == 192 || NN == 64 || NN == 80)) ||
           (H == 96 && (NN == 288 || NN == 80 || NN == 96));
}
static bool old_src_fused_supported(int H, int N) { return (H == 32 && N == 96) || (H == 64 && N == 192) || (H == 96 && N == 288); }
static int old_npad(int N) { return (N + 63) / 64 * 64; }
static int old_tfl_rb(int B, int N, const Switches& s) {
    if (s.tfl_rb) return s.tfl_rb;
    const long tiles16 = (long)B * (old_npad(N) / 16);
    return tiles16 >= 4 * 256 ? 4 : (tiles16 > 256 ? 2 : 1);
}
static int old_ntile(int N, int rb) { return (old_npad(N) + 16 * rb - 1) / (16 * rb); }
static int old_tf_waves(int R, const Switches& s) {
    if (s.tf_waves) return s.tf_waves;
    return (R + 31) / 32 < 2 * 256 ? 8 : 4;
}
static bool old_tfl_use(const OldTfCall& c, const Switches& s) {
    return s.tf_layer && c.tfused && !c.att_f32 && c.n > 0 && old_tfl_supported(c.H, c.heads);
}
static bool old_tf_chain(const OldTfCall& c, const Switches& s) {
    return s.tf_chain && c.tfused && old_post_next_supported(c.H, 3 * c.H);
}
static OldTf old_transformer(const OldTfCall& c, const Switches& s) {
    OldTf o;
    const int H = c.H, n = c.n, R = c.B * c.N;
    o.form = old_tfl_use(c, s) ? 3 : (!c.tfused ? 0 : (old_tf_chain(c, s) ? 2 : 1));  // m2_debug_transformer_form
    if (c.B == 0 || c.N == 0) return o;
    if (c.devT && !(old_tfl_use(c, s) && old_tfl_proj_supported(H, c.mel))) {
        o.err = M2_E_ARG, o.msg = "mel decoder: a device frame count needs the one-launch layers";
        return o;
    }
    if (c.ragged && !old_tfl_use(c, s)) {
        o.err = M2_E_SHAPE, o.msg = "mel decoder: per-utterance frame counts need the one-launch layers "
                                    "(hidden_dim 32 / 64 / 96 with 2 heads, M2_TF_LAYER not 0)";
        return o;
    }
    auto plain = [&](const char* kind, int layer, int op = 0) { o.rows.push_back({kind, layer, 0, op, 0, 0, 0, 0, 0}); };
    auto gemm = [&](const char* kind, int layer, int next = 0) {  // launch_ln_gemm / launch_post_attn*: tf_waves, 32-row tiles
        const int nw = old_tf_waves(R, s);
        o.rows.push_back({kind, layer, next, 0, 0, 0, nw, (R + 31) / 32, 64 * nw});
    };
    auto final_projection = [&] {
        if (c.mel == 0) return;  // text_encoder_layers ends with the layers
        if (c.tfused && old_post_next_supported(H, c.mel)) gemm("final_ln_gemm", n);
        else plain("final_linear", n);
    };
    if (old_tfl_use(c, s)) {
        {  // launch_tfl_first
            int rb = old_tfl_rb(c.B, c.N, s) > 1 ? 2 : 1;
            if ((long)c.B * (old_npad(c.N) / 16) >= 8L * 256) rb = 4;
            if (s.tfl_first_rb) rb = s.tfl_first_rb;
            if (c.masked && s.tfl_rb_masked) rb = s.tfl_rb_masked;
            if (!c.masked && s.tfl_rb_unmasked) rb = s.tfl_rb_unmasked;
            o.rows.push_back({"tfl_first", 0, 0, 0, rb, 0, 0, c.B * old_ntile(c.N, rb), (rb == 4 ? 4 : 8) * 64});
        }
        for (int l = 0; l < n; ++l) {  // run_tfl, launch_tfl_layer
            const int next = l + 1 < n ? 1 : (c.mel > 0 && old_tfl_proj_supported(H, c.mel) ? 2 : 0);
            const int rb = c.masked && s.tfl_rb_masked ? s.tfl_rb_masked
                           : !c.masked && s.tfl_rb_unmasked ? s.tfl_rb_unmasked : old_tfl_rb(c.B, c.N, s);
            int qs2 = s.tfl_qs2 >= 0 ? s.tfl_qs2 : 12;
            if (qs2 == 12 && (c.masked || (c.wide_last && l == n - 1))) qs2 = H / 2 >= 48 ? 3 : 4;
            o.rows.push_back({"tfl_layer", l, next, 0, rb, qs2, 0, c.B * old_ntile(c.N, rb), 8 * 64});
            if (next == 2) o.projected = true;
        }
        if (!o.projected) final_projection();
        return o;
    }
    const bool chain = old_tf_chain(c, s);
    const bool first_fused = chain && n > 0 && old_src_fused_supported(H, 3 * H);
    bool qkv_ready = false;
    if (c.src == 1) {
        if (first_fused) gemm("embed_ln_gemm", 0), qkv_ready = true;
        else plain("embed_pe", 0);
    } else if (c.src == 2) {
        if (first_fused) gemm("expand_ln_gemm", 0), qkv_ready = true;
        else plain("lr_expand", 0);
    }
    if (!chain) {  // run_stack -> run_layer
        for (int l = 0; l < n; ++l) {
            if (c.tfused) {
                gemm("ln_gemm", l);
                plain("attention", l);
                gemm("post_attn", l);
            } else {
                plain("linear", l, 0);
                plain("attention", l);
                for (int op = 1; op < 4; ++op) plain("linear", l, op);
            }
        }
    } else if (n > 0) {
        if (!qkv_ready) gemm("ln_gemm", 0);
        for (int l = 0; l < n; ++l) {
            plain("attention", l);
            if (l + 1 < n) gemm("post_attn_next", l, 1);
            else if (c.mel > 0 && old_post_next_supported(H, c.mel)) gemm("post_attn_next", l, 2), o.projected = true;
            else gemm("post_attn", l);
        }
    }
    if (!o.projected) final_projection();
    return o;
}

// The old rules' sequence in the printed format of transformer_plan.h (the pinned lines come from here).
static std::string old_tf_line(const OldTfCall& c, const OldTf& o) {
    char b[256];
    static const char* const src[] = {"x", "embed", "expand"};
    std::snprintf(b, sizeof b, "%s form=%d H=%d heads=%d layers=%d B=%d N=%d src=%s masked=%d devT=%d ragged=%d projected=%d",
                  c.mel ? "dec" : "enc", o.form, c.H, c.heads, c.n, c.B, c.N, src[c.src], (int)c.masked, (int)c.devT,
                  (int)c.ragged, (int)o.projected);
    std::string line = b;
    if (o.err) line += std::string(" error=\"") + o.msg + "\"";
    for (const OldTfRow& r : o.rows) {
        const std::string k = r.kind;
        if (k == "embed_pe" || k == "lr_expand" || k == "final_linear") std::snprintf(b, sizeof b, " %s", r.kind);
        else if (k == "attention") std::snprintf(b, sizeof b, " %s%d", r.kind, r.layer);
        else if (k == "linear") std::snprintf(b, sizeof b, " %s%d[op=%d]", r.kind, r.layer, r.op);
        else if (k == "final_ln_gemm") std::snprintf(b, sizeof b, " %s[waves=%d grid=%d thr=%d]", r.kind, r.waves, r.grid, r.thr);
        else if (k == "post_attn_next")
            std::snprintf(b, sizeof b, " %s%d[next=%d waves=%d grid=%d thr=%d]", r.kind, r.layer, r.next, r.waves, r.grid, r.thr);
        else if (k == "tfl_first") std::snprintf(b, sizeof b, " %s%d[rb=%d grid=%d thr=%d]", r.kind, r.layer, r.rb, r.grid, r.thr);
        else if (k == "tfl_layer")
            std::snprintf(b, sizeof b, " %s%d[next=%d rb=%d qs2=%d grid=%d thr=%d]", r.kind, r.layer, r.next, r.rb, r.qs2, r.grid, r.thr);
        else std::snprintf(b, sizeof b, " %s%d[waves=%d grid=%d thr=%d]", r.kind, r.layer, r.waves, r.grid, r.thr);
        line += b;
    }
    return line;
}

static long g_tf_plans = 0, g_tf_diff = 0, g_tf_inv = 0;

static void check_tf_plan(const OldTfCall& oc, const Switches& s) {
    TfCall c;
    if (oc.n > 0 && oc.wide_last) c.set_wide(oc.n - 1);
    c.decoder = oc.mel > 0;
    c.H = oc.H, c.heads = oc.heads, c.layers = oc.n, c.proj = oc.mel;
    c.tfused = oc.tfused, c.att_f32 = oc.att_f32;
    c.src = (TfSrc)oc.src;
    c.masked = oc.masked, c.device_T = oc.devT, c.ragged = oc.ragged;
    c.B = oc.B, c.N = oc.N;
    const TfPlan p = plan_transformer(c, s);
    const OldTf o = old_transformer(oc, s);
    ++g_tf_plans;
    bool same = p.form == o.form && p.error.code == o.err && (p.error.text == nullptr) == (o.msg == nullptr) &&
                (!o.msg || !std::strcmp(p.error.text, o.msg)) && p.projected == o.projected &&
                p.rows.size() == o.rows.size();
    for (size_t i = 0; same && i < o.rows.size(); ++i) {
        const TfRow& r = p.rows[i];
        const OldTfRow& q = o.rows[i];
        same = !std::strcmp(kTfKindNames[(int)r.kind], q.kind) && r.layer == q.layer && r.next == q.next && r.op == q.op &&
               r.rb == q.rb && r.qs2 == q.qs2 && r.waves == q.waves && r.grid == q.grid && r.threads == q.thr;
    }
    bool inv = true;
    int endings = 0, fused_end = 0;
    for (const TfRow& r : p.rows) {
        const bool has_grid = r.waves > 0 || r.rb > 0;
        inv = inv && (!has_grid || (r.grid >= 1 && r.threads >= 64 && r.threads % 64 == 0 && r.threads <= 1024));
        inv = inv && (has_grid || (r.grid == 0 && r.threads == 0));
        endings += r.kind == TfKind::FinalLnGemm || r.kind == TfKind::FinalLinear;
        fused_end += r.next == 2;
    }
    const bool runs = oc.B > 0 && oc.N > 0 && !p.error.code;
    // a form-3 plan: the first launch, one launch per layer, and an ending of its own exactly when a
    // projection is asked for (the decoder) and the last layer did not run it
    if (runs && p.form == 3) inv = inv && (int)p.rows.size() == 1 + oc.n + (oc.mel > 0 && !p.projected ? 1 : 0);
    inv = inv && p.projected == (fused_end == 1) && fused_end <= 1;
    if (runs) inv = inv && endings == (oc.mel > 0 && !p.projected ? 1 : 0);
    else inv = inv && p.rows.empty() && !p.projected;
    char line[2048];
    const int len = p.print(line, sizeof line);
    inv = inv && len > 0 && len < (int)sizeof line && (int)std::strlen(line) == len;
    same = same && old_tf_line(oc, o) == line;
    if ((!same || !inv) && g_tf_diff + g_tf_inv < 5)
        std::printf("  %s%s| %s\n    old: %s\n", same ? "" : "DIFFERS ", inv ? "" : "INVARIANT ", line, old_tf_line(oc, o).c_str());
    g_tf_diff += !same;
    g_tf_inv += !inv;
}

static void expect_tf_line(const char* what, const OldTfCall& oc, const char* want) {
    const std::string got = old_tf_line(oc, old_transformer(oc, Switches{}));
    const bool ok = got == want;
    std::printf("  %s: %s%s\n", what, got.c_str(), ok ? "" : " (UNEXPECTED)");
    g_bad += !ok;
    check_tf_plan(oc, Switches{});  // and the planner prints the same line
}

static void check_transformer_plan() {
    std::vector<Switches> sws(1);
    auto with = [&](auto set) {
        Switches s;
        set(s);
        sws.push_back(s);
    };
    with([](Switches& s) { s.tf_layer = false; });
    with([](Switches& s) { s.tf_chain = false; });
    with([](Switches& s) { s.tf_layer = s.tf_chain = false; });
    for (const int v : {4, 8}) with([v](Switches& s) { s.tf_waves = v; });
    for (const int v : {1, 2, 4}) {
        with([v](Switches& s) { s.tfl_rb = v; });
        with([v](Switches& s) { s.tfl_first_rb = v; });
        with([v](Switches& s) { s.tfl_rb_masked = v; });
        with([v](Switches& s) { s.tfl_rb_unmasked = v; });
    }
    for (const int v : {0, 2, 3, 4, 12}) with([v](Switches& s) { s.tfl_qs2 = v; });
    with([](Switches& s) { s.tfl_rb = 4, s.tfl_first_rb = 1, s.tfl_rb_masked = 2; });  // the overrides' order
    // B x N on both sides of each threshold: 256 / 1024 sixteen-row tiles (16, 17, 64 x 256), 2048
    // (128 x 256), 512 thirty-two-row tiles (127, 128 x 128); 0: the empty call
    const int Bs[] = {0, 1, 2, 16, 17, 64, 127, 128}, Ns[] = {0, 1, 63, 64, 65, 128, 256, 500, 2600};
    struct Mode {
        bool devT, ragged;
    };
    const Mode modes[] = {{false, false}, {true, false}, {false, true}, {true, true}};
    for (const int H : {32, 48, 64, 96, 128})
        for (const int heads : {1, 2, 3, 4, 6})
            for (const int mel : {0, 32, 40, 48, 64, 80, 96})
                for (const int n : {0, 1, 2, 3})
                    for (int flags = 0; flags < 8; ++flags) {
                        const bool tfused = flags & 1, att_f32 = flags & 2, wide_last = flags & 4;
                        // the geometry rules read (B, N, H, heads, masked, wide, switches) and not the
                        // rest of the handle: every B x N on the fused two-layer handles; on every
                        // handle (every layer count and form) the shapes on both sides of each tile
                        // threshold, a small one and an empty one
                        const bool all_shapes = n == 2 && tfused && !att_f32;
                        for (const int B : Bs)
                            for (const int N : Ns) {
                                const bool threshold = (N == 256 && (B == 16 || B == 17 || B == 64 || B == 128)) ||
                                                       (N == 128 && (B == 127 || B == 128));
                                if (!all_shapes && !(threshold || (B == 2 && N == 65) || (B == 0 && N == 63))) continue;
                                for (int src = 0; src < 3; ++src)
                                    for (int masked = 0; masked < 2; ++masked)
                                        for (const Mode& md : modes) {
                                            // (a device T or ragged rows change the refusal and no geometry)
                                            if ((md.devT || md.ragged) && !(B == 0 || B == 2 || B == 17 || (all_shapes && B == 128)))
                                                continue;
                                            const OldTfCall c{H, heads, n, mel, tfused, att_f32, wide_last, src, masked != 0,
                                                              md.devT, md.ragged, B, N};
                                            for (const Switches& s : sws) check_tf_plan(c, s);
                                        }
                            }
                    }
    std::printf("transformer plans: %ld plans over %zu switch tables, %ld differ from the old rules, %ld break an invariant\n",
                g_tf_plans, sws.size(), g_tf_diff, g_tf_inv);
    g_bad += (int)(g_tf_diff + g_tf_inv);
    // three calls' lines, literally (default switches, no wide layer)
    expect_tf_line("stage1 encoder B=32 S=100 masked", OldTfCall{64, 2, 2, 0, true, false, false, 1, true, false, false, 32, 100},
                   "enc form=3 H=64 heads=2 layers=2 B=32 N=100 src=embed masked=1 devT=0 ragged=0 projected=0 "
                   "tfl_first0[rb=1 grid=256 thr=512] tfl_layer0[next=1 rb=1 qs2=4 grid=256 thr=512] "
                   "tfl_layer1[next=0 rb=1 qs2=4 grid=256 thr=512]");
    expect_tf_line("stage1 decoder B=32 cap 500 devT", OldTfCall{64, 2, 2, 64, true, false, false, 2, false, true, false, 32, 500},
                   "dec form=3 H=64 heads=2 layers=2 B=32 N=500 src=expand masked=0 devT=1 ragged=0 projected=1 "
                   "tfl_first0[rb=2 grid=512 thr=512] tfl_layer0[next=1 rb=4 qs2=12 grid=256 thr=512] "
                   "tfl_layer1[next=2 rb=4 qs2=12 grid=256 thr=512]");
    expect_tf_line("stage2 decoder B=16 T=2600 ragged", OldTfCall{96, 2, 3, 80, true, false, false, 0, false, false, true, 16, 2600},
                   "dec form=3 H=96 heads=2 layers=3 B=16 N=2600 src=x masked=0 devT=0 ragged=1 projected=1 "
                   "tfl_first0[rb=4 grid=656 thr=256] tfl_layer0[next=1 rb=4 qs2=12 grid=656 thr=512] "
                   "tfl_layer1[next=1 rb=4 qs2=12 grid=656 thr=512] tfl_layer2[next=2 rb=4 qs2=12 grid=656 thr=512]");
}

int main() {
    check_strips();
    check_launch_plans();
    check_transformer_plan();
    check_disc_plans();
    check_geometries();
    check_spectral_bwd();
    check_vocoder_grad();
    check_decoder_grad();
    check_encoder_grad();
    check_duration_grad();
    const m2_config stage1{256, 64, 64, 2, 2, 2, 128, 1000}, stage2{256, 96, 80, 3, 3, 2, 256, 1000};
    for (const bool huge : {false, true}) {
        check(2 * huge, "stage1", stage1, huge);
        check(2 * huge + 1, "stage2", stage2, huge);
    }
    std::printf("plan_check: %d unexpected\n", g_bad);
    return g_bad ? 1 : 0;
}
