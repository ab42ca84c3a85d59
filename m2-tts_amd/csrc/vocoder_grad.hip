// The training side of SimpleVocoder: a forward that keeps a tape, from the 28 raw parameters
// (no model handle: an optimizer step changes every one of them), and the gradient with respect
// to those parameters and the input mel.  Exact f32 throughout, no floating-point atomics: every
// reduction over (utterance, position) goes through partials in the workspace that are added in
// a fixed order, so equal inputs give equal bits, and d_mel has no reduction over the batch.
//
//   forward   the per-op path of a stand-alone SimpleVocoder (launch_conv, launch_convT of
//             vocoder.hip with their fused activation and residual), each layer writing its
//             output into the tape (vocoder_grad_plan.h states the maps).
//   backward  plan_steps() in order.  Three kernels of its own:
//             voc_out_bwd_kernel    tanh', the output conv's data gradient and its weight and
//                                   bias partials in one pass over g_y, y and x4; g_z stays in LDS.
//             voc_res_dx_kernel     the resblock's data gradient: g_v = leaky'(lv) conv2^T(g_r),
//                                   g_u = leaky'(a) (g_r + conv1^T(g_v)); conv2^T(g_r) and g_a
//                                   never leave the workgroup.
//             voc_dw_narrow_kernel  weight and bias partials of a Conv1d with fewer than 16
//                                   output channels: a workgroup owns chunks of positions and
//                                   accumulates every (co, ci, tap) product of them.
//             The rest through losses.hip's launchers (conv_launch.h): the ConvTranspose1d's
//             data gradient is conv1d(g_u, WT read as [Cin_T, Cout_T, 2r], stride r, padding
//             r / 2) and its weight gradient is that Conv1d's with input g_u and dy x_k; the
//             wide weight gradients and the input conv on the exact-f32 MFMA.
// The three kernels use fmaf, not the MFMA: they are bound by their loads and stores (the chain
// is about 30 GFLOP at B = 32, T = 500), and the exact-f32 MFMA issues at the vector rate.
#include <algorithm>
#include <cstring>

#include "audio_dsp.h"
#include "conv_launch.h"
#include "vocoder_grad_plan.h"

namespace m2 {
namespace vgrad {

using dsp::block_sum;

__device__ __forceinline__ float leaky_d(float stored) { return stored > 0.f ? 1.f : kLeaky; }

// grid (cdiv(L, kOutP), B), 256 threads, (kOutP + 2) floats of LDS.  y = tanh(z),
// z = conv(x [B, c, L]; w [1, c, 3], padding 1) + b; gy, y [B, 1, L].  g_z = gy (1 - y^2) of the
// workgroup's positions and one more on each side (0 outside [0, L)) is formed in LDS; then per
// input channel gx[ci][p] = sum_tap w[ci][tap] g_z[p + 1 - tap] (or gx null) and the partials
// dw[ci][tap] = sum_p g_z[p] x[ci][p - 1 + tap], db = sum_p g_z[p] over the workgroup's own
// positions: partW [B x chunks, 3 c], partB [B x chunks] (either may be null), slot b chunks + chunk.
__global__ __launch_bounds__(256) void voc_out_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ y,
                                                          const float* __restrict__ x, const float* __restrict__ w,
                                                          int c, int L, float* __restrict__ gx,
                                                          float* __restrict__ partW, float* __restrict__ partB) {
    extern __shared__ float gz[];
    __shared__ double red[4];
    const int tid = threadIdx.x, b = blockIdx.y, p0 = blockIdx.x * kOutP;
    const float* gyb = gy + (size_t)b * L;
    const float* yb = y + (size_t)b * L;
    for (int i = tid; i < kOutP + 2; i += 256) {
        const int p = p0 - 1 + i;
        float v = 0.f;
        if (p >= 0 && p < L) {
            const float t = yb[p];
            v = gyb[p] * (1.f - t * t);
        }
        gz[i] = v;
    }
    __syncthreads();
    const size_t slot = (size_t)b * gridDim.x + blockIdx.x;
    if (partB) {  // the same for every thread of the workgroup
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < kOutP / 256; ++j) s += gz[tid + 256 * j + 1];
        const double t = block_sum((double)s, red);
        if (tid == 0) partB[slot] = (float)t;
    }
    for (int ci = 0; ci < c; ++ci) {
        const size_t row = ((size_t)b * c + ci) * L;
        const float* xr = x + row;
        const float w0 = w[ci * 3], w1 = w[ci * 3 + 1], w2 = w[ci * 3 + 2];
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < kOutP / 256; ++j) {
            const int i = tid + 256 * j, p = p0 + i;
            if (p < L) {
                const float g = gz[i + 1];
                if (gx) gx[row + p] = fmaf(w2, gz[i], fmaf(w1, g, w0 * gz[i + 2]));
                if (partW) {
                    s0 = fmaf(g, p > 0 ? xr[p - 1] : 0.f, s0);
                    s1 = fmaf(g, xr[p], s1);
                    s2 = fmaf(g, p + 1 < L ? xr[p + 1] : 0.f, s2);
                }
            }
        }
        if (partW) {
            const double t0 = block_sum((double)s0, red), t1 = block_sum((double)s1, red),
                         t2 = block_sum((double)s2, red);
            if (tid == 0) {
                float* o = partW + slot * 3 * c + ci * 3;
                o[0] = (float)t0;
                o[1] = (float)t1;
                o[2] = (float)t2;
            }
        }
    }
}

// grid (cdiv(L, W - 2), B), 256 threads, c (2 W + 2) floats of LDS; W = res_width(c), a power of
// two.  x_out = conv2(lv) + a, lv = leaky(conv1(a)), a = leaky(u); every map [B, c, L], w1 and w2
// [c, c, 3] with padding 1.  A workgroup owns the positions [p0, p0 + W - 2), p0 = (W - 2) bx.  It
// stages g_r on [p0 - 2, p0 + W) (0 outside [0, L)), forms
//   g_v[ci][p] = leaky'(lv[ci][p]) sum_co sum_tap w2[co][ci][tap] g_r[co][p + 1 - tap]
// on [p0 - 1, p0 + W - 1) in LDS (0 outside [0, L): conv1 pads its input with zeros), then on its
// own positions
//   g_u[ci][p] = leaky'(a[ci][p]) (g_r[ci][p] + sum_co sum_tap w1[co][ci][tap] g_v[co][p + 1 - tap])
// and writes g_v and g_u.  Thread t takes window column t % W and the channels t / W, + 256 / W, ...
__global__ __launch_bounds__(256) void voc_res_dx_kernel(const float* __restrict__ g_r, const float* __restrict__ lv,
                                                         const float* __restrict__ a, const float* __restrict__ w1,
                                                         const float* __restrict__ w2, int c, int L, int W,
                                                         float* __restrict__ g_v, float* __restrict__ g_u) {
    extern __shared__ float sm[];
    const int Wr = W + 2;
    float* grs = sm;                    // [c][W + 2]: positions p0 - 2 + o
    float* gvs = sm + (size_t)c * Wr;   // [c][W]: positions p0 - 1 + i
    const int tid = threadIdx.x, b = blockIdx.y, p0 = blockIdx.x * (W - 2);
    const size_t base = (size_t)b * c * L;
    for (int i = tid; i < c * Wr; i += 256) {
        const int ch = i / Wr, o = i - ch * Wr, q = p0 - 2 + o;
        grs[i] = (q >= 0 && q < L) ? g_r[base + (size_t)ch * L + q] : 0.f;
    }
    __syncthreads();
    const int col = tid & (W - 1), cg = tid / W, ncg = 256 / W;
    const int p = p0 - 1 + col;
    const bool in = p >= 0 && p < L;
    for (int ci = cg; ci < c; ci += ncg) {
        float s = 0.f;
        if (in) {
            const float* gr = grs + col;
            const float* wr = w2 + (size_t)ci * 3;
            for (int co = 0; co < c; ++co, gr += Wr, wr += (size_t)c * 3) {
                s = fmaf(wr[0], gr[2], s);
                s = fmaf(wr[1], gr[1], s);
                s = fmaf(wr[2], gr[0], s);
            }
            s *= leaky_d(lv[base + (size_t)ci * L + p]);
        }
        gvs[ci * W + col] = s;
    }
    __syncthreads();
    if (col < 1 || col >= W - 1 || p >= L) return;
    for (int ci = cg; ci < c; ci += ncg) {
        float s = 0.f;
        const float* gv = gvs + col;
        const float* wr = w1 + (size_t)ci * 3;
        for (int co = 0; co < c; ++co, gv += W, wr += (size_t)c * 3) {
            s = fmaf(wr[0], gv[1], s);
            s = fmaf(wr[1], gv[0], s);
            s = fmaf(wr[2], gv[-1], s);
        }
        const size_t i = base + (size_t)ci * L + p;
        g_u[i] = (grs[ci * Wr + col + 1] + s) * leaky_d(a[i]);
        g_v[i] = gvs[ci * W + col];
    }
}

// grid (splits), 256 threads.  The partials of dw[co][ci][tap] = sum over (utterance, t) of
// dy[co][t] x[ci][t stride + tap - pad] and of db[co] = sum dy[co][t], for a Conv1d without groups
// and fewer than 16 output channels; x [nb, Cin, L] as the conv read it, dy [nb, Cout, Lo].  K
// runs over (utterance, output position) in chunks of kNwP positions, workgroup z the chunks
// [z cps, (z + 1) cps): dy[Cout][kNwP] and the input window of those positions are staged in
// LDS; wave w takes the elements w, w + 4, ..., its lanes the positions, an xor-shuffle tree sums
// them and lane 0 adds the chunk's sum to the element's accumulator in LDS.
// partW [splits, Cout Cin k]; partB [splits, Cout] or null.
__global__ __launch_bounds__(256) void voc_dw_narrow_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                            ConvGeo g, int nb, int L, int Lo, int cps,
                                                            float* __restrict__ partW, float* __restrict__ partB) {
    extern __shared__ float sm[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = g.Cout * g.Cin * g.k, ne = n + (partB ? g.Cout : 0);
    const int span = (kNwP - 1) * g.stride + g.k;
    float* dys = sm;                          // [Cout][kNwP]
    float* xs = dys + g.Cout * kNwP;          // [Cin][span]
    float* acc = xs + (size_t)g.Cin * span;   // [n + Cout]
    for (int e = tid; e < ne; e += 256) acc[e] = 0.f;
    const int tcn = (Lo + kNwP - 1) / kNwP, total = nb * tcn;
    const int ch1 = min(total, ((int)blockIdx.x + 1) * cps);
    for (int ch = blockIdx.x * cps; ch < ch1; ++ch) {
        const int b = ch / tcn, t0 = (ch - b * tcn) * kNwP, nt = min(kNwP, Lo - t0);
        __syncthreads();
        const float* dyb = dy + (size_t)b * g.Cout * Lo;
        for (int i = tid; i < g.Cout * kNwP; i += 256) {
            const int co = i / kNwP, tt = i - co * kNwP;
            dys[i] = tt < nt ? dyb[(size_t)co * Lo + t0 + tt] : 0.f;
        }
        const float* xb = x + (size_t)b * g.Cin * L;
        const long long i0 = (long long)t0 * g.stride - g.pad;
        for (int i = tid; i < g.Cin * span; i += 256) {
            const int ci = i / span, o = i - ci * span;
            const long long pos = i0 + o;
            xs[i] = (pos >= 0 && pos < L) ? xb[(size_t)ci * L + pos] : 0.f;
        }
        __syncthreads();
        for (int e = wave; e < ne; e += 4) {
            float s = 0.f;
            if (e < n) {
                const int co = e / (g.Cin * g.k), rem = e - co * g.Cin * g.k, ci = rem / g.k, tap = rem - ci * g.k;
                const float* dr = dys + co * kNwP;
                const float* xr = xs + ci * span + tap;
                for (int tt = lane; tt < nt; tt += 64) s = fmaf(dr[tt], xr[tt * g.stride], s);
            } else {
                const float* dr = dys + (e - n) * kNwP;
                for (int tt = lane; tt < nt; tt += 64) s += dr[tt];
            }
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if (lane == 0) acc[e] += s;
        }
    }
    __syncthreads();
    for (int e = tid; e < ne; e += 256) {
        if (e < n) partW[(size_t)blockIdx.x * n + e] = acc[e];
        else partB[(size_t)blockIdx.x * g.Cout + (e - n)] = acc[e];
    }
}

// dst[i] += src[i]: the one fp32 addition of `accumulate`.
__global__ __launch_bounds__(256) void voc_add_kernel(const float* __restrict__ src, size_t n, float* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] += src[i];
}

}  // namespace vgrad
}  // namespace m2

namespace {
using namespace m2;
using vgrad::Dims;
using vgrad::LaunchRow;
using vgrad::Step;

dim3 grid_of(const LaunchRow& r) { return dim3(r.gx, r.gy, r.gz); }

// voc_out_bwd_kernel and the finishes of its partials; part holds out_part_floats.
int32_t launch_out_bwd(const float* gy, const float* y, const float* x, const float* w, int nb, int c, int L, float* gx,
                       float* dw, float* db, float* part, hipStream_t st) {
    const LaunchRow r = vgrad::out_row(nb, L);
    const int slots = nb * vgrad::out_chunks(L);
    float* partW = dw ? part : nullptr;
    float* partB = db ? part + (size_t)slots * 3 * c : nullptr;
    hipLaunchKernelGGL(vgrad::voc_out_bwd_kernel, grid_of(r), dim3(r.threads), r.lds, st, gy, y, x, w, c, L, gx, partW,
                       partB);
    M2_LAUNCHED(r.kernel);
    if (dw) {
        const int32_t rc = loss::launch_dw_finish(partW, (size_t)3 * c, slots, false, dw, st);
        if (rc != M2_OK) return rc;
    }
    if (db) return loss::launch_dw_finish(partB, 1, slots, false, db, st);
    return M2_OK;
}

int32_t launch_res_dx(const float* g_r, const float* lv, const float* a, const float* w1, const float* w2, int nb, int c,
                      int L, float* g_v, float* g_u, hipStream_t st) {
    const LaunchRow r = vgrad::res_row(c, nb, L);
    hipLaunchKernelGGL(vgrad::voc_res_dx_kernel, grid_of(r), dim3(r.threads), r.lds, st, g_r, lv, a, w1, w2, c, L,
                       vgrad::res_width(c), g_v, g_u);
    M2_LAUNCHED(r.kernel);
    return M2_OK;
}

// voc_dw_narrow_kernel and the finishes; part holds narrow_plan's part_floats.
int32_t launch_narrow_dw(const float* x, const float* dy, const loss::ConvGeo& g, int nb, int L, float* dw, float* db,
                         float* part, hipStream_t st) {
    const vgrad::NarrowPlan p = vgrad::narrow_plan(g, nb, L);
    if (!p.ok) return fail(M2_E_INTERNAL, "voc_dw_narrow_kernel: the plan does not fit");
    const size_t n = (size_t)g.Cout * g.Cin * g.k;
    float* partB = db ? part + (size_t)p.splits * n : nullptr;
    hipLaunchKernelGGL(vgrad::voc_dw_narrow_kernel, dim3(p.splits), dim3(256), p.lds, st, x, dy, g, nb, L,
                       loss::conv_out_len(L, g), p.cps, part, partB);
    M2_LAUNCHED("voc_dw_narrow_kernel");
    if (dw) {
        const int32_t rc = loss::launch_dw_finish(part, n, p.splits, false, dw, st);
        if (rc != M2_OK) return rc;
    }
    if (db) return loss::launch_dw_finish(partB, (size_t)g.Cout, p.splits, false, db, st);
    return M2_OK;
}

int32_t launch_add(const float* src, size_t n, float* dst, hipStream_t st) {
    hipLaunchKernelGGL(vgrad::voc_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, n, dst);
    M2_LAUNCHED("voc_add_kernel");
    return M2_OK;
}

size_t tape_bytes(const Dims& d) {
    Sizer s;
    vgrad::carve_tape(s, d, nullptr);
    return s.off + 256;
}

size_t backward_bytes(const Dims& d) {
    if (d.B == 0 || d.T == 0) return 256;
    Sizer s;
    vgrad::carve_backward(s, d, nullptr);
    return s.off + 256;
}
}  // namespace

extern "C" {

size_t m2_vocoder_tape_bytes(int32_t M, int32_t C, int32_t B, int32_t T) {
    const Dims d{M, C, B, T};
    return vgrad::dims_ok(d) ? tape_bytes(d) : 0;
}

int32_t m2_vocoder_tape_map(int32_t M, int32_t C, int32_t B, int32_t T, int32_t index, size_t* offset_floats,
                            int32_t* channels, int32_t* length) {
    const Dims d{M, C, B, T};
    M2_CHECK_ARG(offset_floats && channels && length && index >= 0 && index < vgrad::kMaps,
                 "m2_vocoder_tape_map: bad argument");
    M2_CHECK_SHAPE(vgrad::dims_ok(d), "m2_vocoder_tape_map: C a multiple of 16 in [16, 256], M >= 1");
    Sizer s;  // carve_tape's arithmetic, map by map
    for (int i = 0; i <= index; ++i) {
        int c, n;
        vgrad::map_shape(d, i, &c, &n);
        const size_t at = align_up(s.off, 256);
        s.take<float>((size_t)d.B * c * n);
        if (i == index) {
            *offset_floats = at / sizeof(float);
            *channels = c;
            *length = n;
        }
    }
    return M2_OK;
}

int32_t m2_vocoder_train_forward(const float* const* params, int32_t M, int32_t C, const float* mel, int32_t B,
                                 int32_t T, float* audio, void* tape, size_t tape_bytes_, void* stream) {
    const Dims d{M, C, B, T};
    M2_CHECK_SHAPE(vgrad::dims_ok(d), "m2_vocoder_train_forward: C a multiple of 16 in [16, 256], M >= 1");
    if (B == 0 || T == 0) return M2_OK;
    M2_CHECK_ARG(params && mel && audio && tape, "m2_vocoder_train_forward: bad argument");
    for (int i = 0; i < vgrad::kParams; ++i) M2_CHECK_ARG(params[i], "m2_vocoder_train_forward: null parameter");
    Carve c(tape, tape_bytes_);
    float* map[vgrad::kMaps];
    vgrad::carve_tape(c, d, map);
    if (!c.ok) return fail(M2_E_ARG, "m2_vocoder_train_forward: tape too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t rc = launch_conv(mel, params[0], params[1], nullptr, nullptr, nullptr, 3, ACT_NONE, false, B, M, C, T,
                             map[vgrad::MAP_H], st);
    for (int k = 0; k < vgrad::kStages && rc == M2_OK; ++k) {
        const int cin = C >> k, ck = vgrad::stage_c(d, k), L = vgrad::stage_len(d, k);
        float *a = map[vgrad::map_a(k)], *lv = map[vgrad::map_lv(k)], *xo = map[vgrad::map_x(k + 1)];
        rc = launch_convT(map[vgrad::map_x(k)], params[vgrad::p_up(k)], params[vgrad::p_up(k) + 1], vgrad::kRates[k],
                          ACT_LEAKY, B, cin, ck, L / vgrad::kRates[k], a, st);
        if (rc == M2_OK)
            rc = launch_conv(a, params[vgrad::p_c1(k)], params[vgrad::p_c1(k) + 1], nullptr, nullptr, nullptr, 3,
                             ACT_LEAKY, false, B, ck, ck, L, lv, st);
        if (rc == M2_OK)
            rc = launch_conv(lv, params[vgrad::p_c2(k)], params[vgrad::p_c2(k) + 1], nullptr, nullptr, a, 3, ACT_NONE,
                             false, B, ck, ck, L, xo, st);
    }
    if (rc != M2_OK) return rc;
    rc = launch_conv(map[vgrad::map_x(vgrad::kStages)], params[vgrad::p_out()], params[vgrad::p_out() + 1], nullptr,
                     nullptr, nullptr, 3, ACT_TANH, false, B, vgrad::stage_c(d, 3), 1, 64 * T, map[vgrad::MAP_Y], st);
    if (rc != M2_OK) return rc;
    M2_HIP(hipMemcpyAsync(audio, map[vgrad::MAP_Y], (size_t)B * 64 * T * sizeof(float), hipMemcpyDeviceToDevice, st));
    return M2_OK;
}

size_t m2_vocoder_backward_workspace_bytes(int32_t M, int32_t C, int32_t B, int32_t T) {
    const Dims d{M, C, B, T};
    return vgrad::dims_ok(d) ? backward_bytes(d) : 0;
}

int32_t m2_vocoder_backward(const float* const* params, int32_t M, int32_t C, const float* mel, int32_t B, int32_t T,
                            const void* tape, const float* d_audio, float* d_mel, float* const* grads,
                            int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    const Dims d{M, C, B, T};
    M2_CHECK_SHAPE(vgrad::dims_ok(d), "m2_vocoder_backward: C a multiple of 16 in [16, 256], M >= 1");
    if (B == 0 || T == 0) return M2_OK;
    M2_CHECK_ARG(params && mel && tape && d_audio && grads && workspace, "m2_vocoder_backward: bad argument");
    for (int i = 0; i < vgrad::kParams; ++i) M2_CHECK_ARG(params[i], "m2_vocoder_backward: null parameter");
    Sizer ts;
    vgrad::carve_tape(ts, d, nullptr);
    Carve tc(const_cast<void*>(tape), ts.off);
    float* map[vgrad::kMaps];
    vgrad::carve_tape(tc, d, map);
    Carve c(workspace, workspace_bytes);
    vgrad::Bufs bufs;
    vgrad::carve_backward(c, d, &bufs);
    if (!c.ok) return fail(M2_E_ARG, "m2_vocoder_backward: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool acc = accumulate != 0;
    auto buf = [&](int id) -> float* {
        switch (id) {
            case vgrad::BUF_NONE: return nullptr;
            case vgrad::BUF_COT0: return bufs.cot[0];
            case vgrad::BUF_COT1: return bufs.cot[1];
            case vgrad::BUF_GV: return bufs.gv;
            case vgrad::BUF_MEL: return const_cast<float*>(mel);
            case vgrad::BUF_DAUDIO: return const_cast<float*>(d_audio);
            case vgrad::BUF_DMEL: return d_mel;
            default: return map[id];
        }
    };
    auto grad = [&](int i) -> float* { return i >= 0 ? grads[i] : nullptr; };
    // with `accumulate` a gradient is formed in the workspace as without it, then added onto the caller's
    for (const Step& s : vgrad::plan_steps(d)) {
        int32_t rc = M2_OK;
        float *const dw_out = grad(s.dw), *const db_out = grad(s.db);
        float* dw = dw_out && acc ? bufs.wtmp : dw_out;
        float* db = db_out && acc ? bufs.btmp : db_out;
        switch (s.kind) {
            case vgrad::STEP_OUT:
                rc = launch_out_bwd(d_audio, map[vgrad::MAP_Y], buf(s.x), params[s.w], B, s.g.Cin, s.L, bufs.cot[0], dw,
                                    db, bufs.part, st);
                break;
            case vgrad::STEP_RES: {
                const int k = s.stage;
                rc = launch_res_dx(bufs.cot[0], map[vgrad::map_lv(k)], map[vgrad::map_a(k)], params[vgrad::p_c1(k)],
                                   params[vgrad::p_c2(k)], B, s.g.Cin, s.L, bufs.gv, bufs.cot[1], st);
                break;
            }
            case vgrad::STEP_WGRAD:
                if (!dw && !db) break;
                if (s.narrow) rc = launch_narrow_dw(buf(s.x), buf(s.dy), s.g, B, s.L, dw, db, bufs.part, st);
                else rc = loss::launch_conv_bwd(buf(s.x), nullptr, buf(s.dy), s.g, B, s.L, false, 1.f, nullptr, dw, db,
                                                false, bufs.part, st);
                break;
            case vgrad::STEP_BIAS:
                if (db) rc = loss::launch_conv_db(buf(s.dy), B, s.g.Cin, s.L, false, db, st);
                break;
            case vgrad::STEP_CONV:
                rc = loss::launch_conv(buf(s.x), params[s.w], nullptr, buf(s.dy), s.g, B, s.L, 1, false, 1.f, 1.f, st);
                break;
            case vgrad::STEP_IN:
                if (d_mel || dw || db)
                    rc = loss::launch_conv_bwd(mel, params[s.w], buf(s.dy), s.g, B, s.L, false, 1.f, d_mel, dw, db, false,
                                               bufs.part, st);
                break;
        }
        if (rc == M2_OK && acc && dw_out) rc = launch_add(bufs.wtmp, vgrad::step_dw_floats(s), dw_out, st);
        if (rc == M2_OK && acc && db_out) rc = launch_add(bufs.btmp, vgrad::step_db_floats(s), db_out, st);
        if (rc != M2_OK) return rc;
    }
    return M2_OK;
}

int32_t m2_debug_vocoder_grad_plan(int32_t M, int32_t C, int32_t B, int32_t T, char* out, size_t cap) {
    const Dims d{M, C, B, T};
    M2_CHECK_ARG(out && cap > 0 && B > 0 && T > 0, "m2_debug_vocoder_grad_plan: bad argument");
    M2_CHECK_SHAPE(vgrad::dims_ok(d), "m2_debug_vocoder_grad_plan: C a multiple of 16 in [16, 256], M >= 1");
    const std::string line = vgrad::print_plan(d);
    const size_t n = std::min(line.size(), cap - 1);
    std::memcpy(out, line.data(), n);
    out[n] = '\0';
    return (int32_t)line.size();
}

// ---- the three kernels alone -------------------------------------------------------

size_t m2_vocoder_out_backward_workspace_bytes(int32_t B, int32_t c, int32_t L) {
    if (B <= 0 || c <= 0 || L <= 0) return 0;
    return vgrad::out_part_floats(c, B, L) * sizeof(float) + 256;
}

int32_t m2_vocoder_out_backward(const float* gy, const float* y, const float* x, const float* w, int32_t B, int32_t c,
                                int32_t L, float* gx, float* dw, float* db, void* workspace, size_t workspace_bytes,
                                void* stream) {
    M2_CHECK_ARG(gy && y && x && w && B >= 0 && c > 0 && L > 0, "m2_vocoder_out_backward: bad argument");
    M2_CHECK_SHAPE(B <= loss::kMaxGrid && c <= (1 << 16) && L <= (1 << 28),
                   "m2_vocoder_out_backward: at most 65535 utterances of 2^28 samples, 2^16 channels");
    if (B == 0) return M2_OK;
    Carve cv(workspace, workspace_bytes);
    float* part = (dw || db) ? cv.take<float>(vgrad::out_part_floats(c, B, L)) : nullptr;
    if (!cv.ok) return fail(M2_E_ARG, "m2_vocoder_out_backward: workspace too small");
    return launch_out_bwd(gy, y, x, w, B, c, L, gx, dw, db, part, static_cast<hipStream_t>(stream));
}

int32_t m2_resblock_backward(const float* g_r, const float* lv, const float* a, const float* w1, const float* w2,
                             int32_t B, int32_t c, int32_t L, float* g_v, float* g_u, void* stream) {
    M2_CHECK_ARG(g_r && lv && a && w1 && w2 && g_v && g_u && B >= 0 && c > 0 && L > 0,
                 "m2_resblock_backward: bad argument");
    M2_CHECK_SHAPE(B <= loss::kMaxGrid && c <= vgrad::kMaxC / 2 && L <= (1 << 28),
                   "m2_resblock_backward: at most 65535 utterances of 2^28 samples, 128 channels");
    if (B == 0) return M2_OK;
    return launch_res_dx(g_r, lv, a, w1, w2, B, c, L, g_v, g_u, static_cast<hipStream_t>(stream));
}

size_t m2_conv1d_narrow_dw_workspace_bytes(int32_t ksize, int32_t stride, int32_t padding, int32_t B, int32_t Cin,
                                           int32_t Cout, int32_t L) {
    if (B <= 0 || L <= 0 || Cin <= 0 || Cout <= 0 || ksize <= 0 || stride <= 0 || padding < 0 ||
        (long long)L + 2LL * padding < ksize)
        return 0;
    const vgrad::NarrowPlan p = vgrad::narrow_plan(loss::ConvGeo{Cin, Cout, ksize, stride, padding, 1}, B, L);
    return p.ok ? p.part_floats * sizeof(float) + 256 : 0;
}

int32_t m2_conv1d_narrow_dw(const float* x, const float* dy, int32_t ksize, int32_t stride, int32_t padding, int32_t B,
                            int32_t Cin, int32_t Cout, int32_t L, float* dw, float* db,
                            void* workspace, size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(x && dy && (dw || db) && B >= 0 && L > 0 && Cin > 0 && Cout > 0 && ksize > 0 && stride > 0 &&
                     padding >= 0,
                 "m2_conv1d_narrow_dw: bad argument");
    M2_CHECK_SHAPE((long long)L + 2LL * padding >= ksize && L <= (1 << 28) && padding <= (1 << 28),
                   "m2_conv1d_narrow_dw: kernel wider than the padded input");
    if (B == 0) return M2_OK;
    const loss::ConvGeo g{Cin, Cout, ksize, stride, padding, 1};
    const vgrad::NarrowPlan p = vgrad::narrow_plan(g, B, L);
    M2_CHECK_SHAPE(p.ok, "m2_conv1d_narrow_dw: fewer than 16 output channels, and the windows must fit 48 KiB of LDS");
    Carve cv(workspace, workspace_bytes);
    float* part = cv.take<float>(p.part_floats);
    if (!cv.ok) return fail(M2_E_ARG, "m2_conv1d_narrow_dw: workspace too small");
    return launch_narrow_dw(x, dy, g, B, L, dw, db, part, static_cast<hipStream_t>(stream));
}

}  // extern "C"
