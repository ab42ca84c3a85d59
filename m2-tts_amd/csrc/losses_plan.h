// The host-only half of losses.hip: the geometry of the discriminators' convs,
// the plans that decide LDS sizes, grids and split counts, and the workspace
// layout of the discriminator calls and of the spectral backward.  Pure arithmetic on the host: nothing
// here touches a device, so tools/plan_check.cpp runs all of it on the CPU.
#pragma once

#include <algorithm>
#include <vector>

#include "m2_common.h"

namespace m2 {
namespace loss {

struct ConvGeo {
    int Cin, Cout, k, stride, pad, groups;
};

constexpr int kNP = 64;          // output positions per conv_mfma workgroup
constexpr int kCoWg = 64;        // output channels per conv_mfma workgroup (4 waves x 16)
constexpr int kCch = 16;         // input channels staged in LDS per step
constexpr int kMaxLds = 48 * 1024;
constexpr int kMaxGrid = 65535;

constexpr int kLayers = 7;
constexpr int kFeat = 6;         // layers whose output is a feature map (more than one channel)
constexpr int kMaxScales = 8;
const ConvGeo kDisc[kLayers] = {{1, 64, 15, 1, 7, 1},       {64, 128, 41, 4, 20, 4},     {128, 256, 41, 4, 20, 16},
                                {256, 512, 41, 4, 20, 64},  {512, 1024, 41, 4, 20, 256}, {1024, 1024, 5, 1, 2, 1},
                                {1024, 1, 3, 1, 1, 1}};

constexpr int kRedChunk = 16384;  // elements per reduce_part_kernel workgroup
constexpr int kRedPart = 4;
constexpr size_t kSliceBytes = (size_t)1 << 30;  // activation bytes a batch slice may take (m2_disc_set_slice_bytes)

constexpr int kDxM = 64;         // column positions per conv_dx_mfma workgroup (4 tiles of 16)
constexpr int kTc = 64;          // output positions staged per conv_dw_mfma step
constexpr int kDwTiles = 11;     // 16-column tiles per wave of conv_dw_mfma
constexpr int kDwCols = 4 * 16 * kDwTiles;  // (input channel, tap) columns per workgroup
constexpr int kDwCiMax = 64;     // input channels per conv_dw_mfma workgroup
constexpr int kMaxSplits = 64;   // split-K partials of one weight gradient
constexpr size_t kPartFloats = (size_t)8 << 20;  // floats the partials of one layer may take (beyond one copy of dw)
constexpr int kAuP = 256;        // pooled positions per conv_dx_audio workgroup
constexpr int kDbThreads = 1024; // threads of a conv_db_kernel workgroup

__host__ __device__ inline int conv_out_len(int L, const ConvGeo& g) { return (L + 2 * g.pad - g.k) / g.stride + 1; }
inline int span_of(const ConvGeo& g) { return (kNP - 1) * g.stride + g.k; }
inline int spanp_of(const ConvGeo& g) { return span_of(g) | 1; }

enum Path { PATH_DIRECT = 0, PATH_MFMA = 1, PATH_WAVE = 2 };
inline Path conv_path(const ConvGeo& g) {
    const int K = g.Cin / g.groups * g.k;
    if (g.Cout >= 16 && K >= 32 && (size_t)kCch * spanp_of(g) * sizeof(float) <= (size_t)kMaxLds) return PATH_MFMA;
    return K >= 256 ? PATH_WAVE : PATH_DIRECT;
}

// Weight element (co, ci in group, tap) is at w[co sCo + ci sCi + tap sK]:
// PyTorch's [Cout, Cin/g, k], or the handle's packed [k, Cin/g, Cout].
struct WStride {
    long long sCo, sCi, sK;
};
inline WStride w_stride(const ConvGeo& g, bool packed) {
    const long long Cg = g.Cin / g.groups;
    return packed ? WStride{1, g.Cout, Cg * g.Cout} : WStride{Cg * g.k, g.k, 1};
}

// How the weight gradient of one layer over nb utterances is computed.
struct DwPlan {
    bool mfma = false;
    int nciB = 0, blocks = 0, splits = 1, cps = 0;
    size_t lds = 0, part_floats = 0;
};

inline DwPlan dw_plan(const ConvGeo& g, int nb, int L) {
    DwPlan p;
    const int Lo = conv_out_len(L, g), Cg = g.Cin / g.groups, Mg = g.Cout / g.groups;
    const long long chunks = (long long)nb * cdiv(Lo, kTc);
    const size_t n = (size_t)g.Cout * Cg * g.k;
    if (g.Cout < 16 || g.k > kDwCols || chunks > (1 << 30)) return p;
    int umax = 0;  // the widest union of input channels over the 16-row tiles
    for (int co0 = 0; co0 < g.Cout; co0 += 16)
        umax = std::max(umax, (std::min(co0 + 15, g.Cout - 1) / Mg + 1 - co0 / Mg) * Cg);
    const size_t spanp = (size_t)(((kTc - 1) * g.stride + g.k) | 1), dys = 16 * (kTc + 1);
    if ((spanp + dys) * sizeof(float) > (size_t)kMaxLds) return p;
    const size_t fit = ((size_t)kMaxLds / sizeof(float) - dys) / spanp;
    p.nciB = (int)std::min<size_t>({(size_t)(kDwCols / g.k), (size_t)kDwCiMax, (size_t)umax, fit});
    p.blocks = cdiv(umax, p.nciB);
    if (p.blocks > kMaxGrid) return p;
    p.mfma = true;
    p.lds = ((size_t)p.nciB * spanp + dys) * sizeof(float);
    const size_t room = 1 + kPartFloats / n;
    p.splits = (int)std::max<long long>(1, std::min<long long>({chunks, (long long)kMaxSplits, (long long)room}));
    p.part_floats = (size_t)p.splits * n;  // before the rounding below: a bound that never shrinks as nb grows
    p.cps = (int)((chunks + p.splits - 1) / p.splits);
    p.splits = (int)((chunks + p.cps - 1) / p.cps);
    return p;
}

// Phases of the stride one conv_dx_mfma workgroup takes (1, 2 or 4; its other waves take row tiles).
inline int dx_phases(const ConvGeo& g) { return g.stride >= 4 ? 4 : g.stride >= 2 ? 2 : 1; }
// conv_dx_mfma_kernel's LDS: dy's window of 16 output channels at an odd row pitch.
inline size_t dx_lds_bytes(const ConvGeo& g) {
    return (size_t)kCch * ((kDxM + (size_t)cdiv(g.k, g.stride) - 1) | 1) * sizeof(float);
}
inline long long dx_grid_y(const ConvGeo& g) {
    return (long long)cdiv(g.stride, dx_phases(g)) * cdiv(g.Cin, 64 / dx_phases(g));
}
inline bool dx_mfma_ok(const ConvGeo& g) {
    return conv_path(g) == PATH_MFMA && g.Cin >= 16 && dx_lds_bytes(g) <= (size_t)kMaxLds && dx_grid_y(g) <= kMaxGrid;
}

// One kernel launch as a launcher issues it: what launch_conv and launch_conv_bwd (losses.hip) launch
// for one layer, in order.  The launchers take their grids and LDS bytes from these rows.
struct LaunchRow {
    const char* kernel;
    unsigned gx, gy, gz;
    int threads;
    size_t lds;
};

// launch_conv over nb utterances of L (pooled) input samples.
inline LaunchRow conv_row(const ConvGeo& g, int nb, int L) {
    const int Lo = conv_out_len(L, g);
    const Path path = conv_path(g);
    if (path == PATH_MFMA)
        return {"conv_mfma_kernel", (unsigned)cdiv(Lo, kNP), (unsigned)cdiv(g.Cout, kCoWg), (unsigned)nb, 256,
                (size_t)kCch * spanp_of(g) * sizeof(float)};
    if (path == PATH_WAVE) return {"conv_wave_kernel", (unsigned)cdiv(Lo, 4), (unsigned)g.Cout, (unsigned)nb, 256, 0};
    return {"conv_direct_kernel", (unsigned)cdiv(Lo, 256), (unsigned)g.Cout, (unsigned)nb, 256, 0};
}

// launch_conv_bwd over nb utterances of L input samples: the data gradient, the weight gradient
// (its partials, then dw_finish_kernel) and the bias gradient, each when asked for.
inline void conv_bwd_rows(const ConvGeo& g, int nb, int L, bool dx, bool dw, bool db, std::vector<LaunchRow>& out) {
    const size_t n = (size_t)g.Cout * (g.Cin / g.groups) * g.k;
    if (dx) {
        if (dx_mfma_ok(g))
            out.push_back({"conv_dx_mfma_kernel", (unsigned)cdiv((L - 1 + g.pad) / g.stride + 1, kDxM),
                           (unsigned)dx_grid_y(g), (unsigned)nb, 256, dx_lds_bytes(g)});
        else
            out.push_back({"conv_dx_direct_kernel", (unsigned)cdiv(L, 256), (unsigned)g.Cin, (unsigned)nb, 256, 0});
    }
    if (dw) {
        const DwPlan p = dw_plan(g, nb, L);
        if (p.mfma) {
            out.push_back({"conv_dw_mfma_kernel", (unsigned)p.blocks, (unsigned)cdiv(g.Cout, 16), (unsigned)p.splits, 256,
                           p.lds});
            out.push_back({"dw_finish_kernel", (unsigned)((n + 255) / 256), 1, 1, 256, 0});
        } else {
            out.push_back({"conv_dw_direct_kernel", (unsigned)n, 1, 1, 256, 0});
        }
    }
    if (db) out.push_back({"conv_db_kernel", (unsigned)g.Cout, 1, 1, kDbThreads, 0});
}

// conv_dx_audio_kernel's LDS: the weights and dy's window of 16 channels.
inline size_t audio_lds_bytes(int Cout, int k) {
    return ((size_t)Cout * k + (size_t)kCch * ((kAuP + k - 1) | 1)) * sizeof(float);
}
inline bool audio_bwd_ok(int Cout, int k) {
    return (long long)Cout * k <= (1 << 13) && k <= (1 << 12) && audio_lds_bytes(Cout, k) <= (size_t)kMaxLds;
}

// Output lengths of the seven layers of the discriminator at `scale`; false when the pooled input is empty.
inline bool disc_lengths(int L, int scale, int len[kLayers]) {
    int l = L / scale;
    if (l < 1) return false;
    for (int i = 0; i < kLayers; ++i) len[i] = l = conv_out_len(l, kDisc[i]);
    return true;
}

// floats of the seven outputs of one utterance at `scale`
inline size_t disc_floats(int L, int scale) {
    int len[kLayers];
    if (!disc_lengths(L, scale, len)) return 0;
    size_t n = 0;
    for (int i = 0; i < kLayers; ++i) n += align_up((size_t)kDisc[i].Cout * len[i], 64);
    return n;
}

// Utterances per batch slice: as many as keep `copies` sets of maps within slice_bytes, at least one.
inline int slice_of(size_t slice_bytes, size_t floats_per_utt, int copies, int B) {
    const size_t per = std::max<size_t>(1, floats_per_utt * copies * sizeof(float));
    const size_t n = slice_bytes / per;
    return (int)std::max<size_t>(1, std::min<size_t>(n, (size_t)std::max(B, 1)));
}

// What one discriminator call over B utterances of L samples walks and carves.  Sizes are floats
// per utterance of a slice (part: of the whole buffer); a size the mode does not use is 0.
enum DiscMode { DISC_FORWARD = 0, DISC_LOSSES = 1, DISC_GEN_STEP = 2, DISC_STEP = 3 };
struct DiscPlan {
    int sides = 1;       // sets of maps resident at once: forward 1, the others real and fake
    int nbs = 1;         // utterances per slice; the last slice may be shorter
    size_t per = 0;      // the seven maps of one side, each rounded up to 64 floats
    size_t layer[kLayers] = {};  // the widest map of each layer over the scales
    int max_chunks = 0;  // reduce_part_kernel's chunk partials per map (the calls that write rows)
    size_t cot = 0;      // the widest map: each of the two cotangent buffers (the steps)
    size_t pooled = 0;   // the pooled audio (the discriminator step, scales above 1)
    size_t part = 0;     // the split-K partials (the discriminator step)
};

inline DiscPlan disc_plan(const int* scales, int n_scales, size_t slice_bytes, int B, int L, DiscMode mode) {
    DiscPlan p;
    for (int s = 0; s < n_scales; ++s) {
        int len[kLayers];
        if (!disc_lengths(L, scales[s], len)) continue;
        p.per = std::max(p.per, disc_floats(L, scales[s]));
        for (int i = 0; i < kLayers; ++i) p.layer[i] = std::max(p.layer[i], (size_t)kDisc[i].Cout * len[i]);
        if (mode == DISC_STEP && scales[s] > 1) p.pooled = std::max(p.pooled, align_up((size_t)(L / scales[s]), 64));
    }
    p.sides = mode == DISC_FORWARD ? 1 : 2;
    p.nbs = slice_of(slice_bytes, p.per, p.sides, B);
    if (mode == DISC_FORWARD) return p;
    p.max_chunks = cdiv((int)std::min<size_t>(p.per, (size_t)1 << 30), kRedChunk) + 1;
    if (mode == DISC_LOSSES) return p;
    for (int i = 0; i < kLayers; ++i) p.cot = std::max(p.cot, align_up(p.layer[i], 64));
    if (mode == DISC_GEN_STEP) return p;
    for (int s = 0; s < n_scales; ++s) {
        int l = L / scales[s];
        if (l < 1) continue;
        // the last slice may be shorter, and fewer utterances never take more partials
        for (int i = 0; i < kLayers; ++i) {
            p.part = std::max(p.part, dw_plan(kDisc[i], p.nbs, l).part_floats);
            l = conv_out_len(l, kDisc[i]);
        }
    }
    return p;
}

struct DiscBufs {
    float* act[2];   // the maps of a slice, side by side: layer i of all its utterances, then layer i + 1
    double* dpart;   // [nbs, kLayers, max_chunks, kRedPart]
    float* cot[2];   // the cotangent of a layer's output and of its input, swapping roles layer by layer
    float* pooled;
    float* part;
};

// The one statement of the discriminator calls' workspace: run over a Sizer it gives the byte
// count, over a Carve the pointers (null where the plan's size is 0).
template <typename A>
void carve_disc(A& a, const DiscPlan& p, DiscBufs* out) {
    const size_t nbs = (size_t)p.nbs;
    auto floats = [&](size_t n) { return n ? a.template take<float>(n) : nullptr; };
    DiscBufs b{};
    for (int side = 0; side < p.sides; ++side) b.act[side] = a.template take<float>(nbs * p.per);
    if (p.max_chunks) b.dpart = a.template take<double>(nbs * kLayers * p.max_chunks * kRedPart);
    for (float*& c : b.cot) c = floats(nbs * p.cot);
    b.pooled = floats(nbs * p.pooled);
    b.part = floats(p.part);
    if (out) *out = b;
}

// m2_loss_spectral_backward's workspace: the frames' cotangents [B, frames, n_fft] between
// spectral_grad_frame_kernel and spectral_fold_kernel (n_fft / hop floats per sample).
inline int spectral_frames(int L, int hop) { return 1 + L / hop; }
template <typename A>
void carve_spectral_bwd(A& a, int n_fft, int hop, int B, int L, float** frames) {
    float* p = a.template take<float>((size_t)B * spectral_frames(L, hop) * n_fft);
    if (frames) *frames = p;
}

}  // namespace loss
}  // namespace m2
