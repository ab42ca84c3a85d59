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
#include <cstdint>
#include <cstdio>

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

int main() {
    check_strips();
    const m2_config stage1{256, 64, 64, 2, 2, 2, 128, 1000}, stage2{256, 96, 80, 3, 3, 2, 256, 1000};
    for (const bool huge : {false, true}) {
        check(2 * huge, "stage1", stage1, huge);
        check(2 * huge + 1, "stage2", stage2, huge);
    }
    std::printf("plan_check: %d unexpected\n", g_bad);
    return g_bad ? 1 : 0;
}
