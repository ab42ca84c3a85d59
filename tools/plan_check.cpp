// The handle's creation plan (csrc/m2_model.h) run on the CPU: no GPU is
// initialised.  Built with the host code under ASan + UBSan by
//   make -C m2-tts_amd/csrc plan_check
// Fills the stage1 and stage2 weight tables from a fixed LCG in +-0.1, plans,
// and prints every decision and pack size; then once more with one vocoder
// and one transformer weight outside the f16 range.  Exit status 1 when a
// flag is not the expected one.
#include <cstdio>

#include "m2_model.h"

using namespace m2;

static int g_bad = 0;

static void expect(const char* what, bool got, bool want) {
    std::printf(" %s=%d%s", what, (int)got, got == want ? "" : "(UNEXPECTED)");
    g_bad += got != want;
}

static void check(const char* stage, const m2_config& c, bool huge) {
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
    // every slot inside its buffer, at the buffer's alignment
    for (const auto& sl : v.f32.slots) g_bad += sl.second % 64 != 0 || sl.second > v.f32.host.size();
    for (const auto& sl : v.split.slots) g_bad += sl.second % 128 != 0 || sl.second > v.split.host.size();
}

int main() {
    const m2_config stage1{256, 64, 64, 2, 2, 2, 128, 1000}, stage2{256, 96, 80, 3, 3, 2, 256, 1000};
    for (const bool huge : {false, true}) {
        check("stage1", stage1, huge);
        check("stage2", stage2, huge);
    }
    std::printf("plan_check: %d unexpected\n", g_bad);
    return g_bad ? 1 : 0;
}
