// The training side of TextEncoder and the length regulator's adjoint: a forward that keeps a tape,
// from the 1 + 11 layers + 2 raw parameters (no model handle), and the gradient with respect to those
// parameters; d_enc of the length regulator given d_reg.  Exact f32, no floating-point atomics: every
// reduction runs in a fixed order, so equal inputs give equal bits (decoder_grad.hip's rules).
//
//   forward   the per-op path of a stand-alone TextEncoder: launch_embed_pe_scaled into the tape's
//             x0, the layers (layer_forward, with the utterances' key mask), launch_layer_norm.
//   backward  encoder_grad_plan.h's plan_steps() in order.  The layers run the decoder's kernels
//             (run_step); the kernels here, all bandwidth-bound:
//             ln_bwd_kernel      the backward of a LayerNorm no linear consumes: lin_dx_kernel's DX_LN
//                                epilogue (ln_bwd_rows) on an accumulator loaded from g_y.
//             emb_dw_kernel      a workgroup owns one vocabulary row and a range of positions, scans
//                                the range's ids and adds the matching rows of d_x0 in ascending
//                                position: nothing is scattered.
//             lr_adjoint_kernel  one wave per phoneme adds its frames of d_reg in ascending order.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "encoder_grad_plan.h"
#include "layer_grad.h"

namespace m2 {

int32_t launch_embed_pe_scaled(const int64_t*, const float*, const float*, int, int, int, int, float, float*, hipStream_t);
int32_t launch_layer_norm(const float*, const float*, const float*, int, int, float*, hipStream_t);

namespace egrad {

using dgrad::f32x4;
using dgrad::kRows;

// grid (cdiv(R, 64)), 256 threads, ln_lds_floats(K).  The cotangent g_y [R, K] of LN(x; gamma, beta),
// x [R, K], K % 8 == 0, K <= 16 KTM <= 128: g_x, and the workgroup's slot of slots [gridDim.x][2 K]
// (ln_bwd_rows; g_res, g_x and slots as there).
template <int KTM>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                     const float* __restrict__ gamma, const float* __restrict__ g_res,
                                                     int R, int K, float* __restrict__ gx, float* __restrict__ slots) {
    extern __shared__ float sm[];
    const int kt = (K + 15) >> 4;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int r0 = blockIdx.x * kRows, lrow = wave * 16 + 4 * g;
    f32x4 acc[KTM];
#pragma unroll
    for (int t = 0; t < KTM; ++t) {
        const int col = 16 * t + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = r0 + lrow + r;
            acc[t][r] = (t < kt && col < K && row < R) ? gy[(size_t)row * K + col] : 0.f;
        }
    }
    dgrad::ln_bwd_rows<KTM>(acc, sm, x, gamma, g_res, R, K, r0, gx,
                            slots ? slots + (size_t)blockIdx.x * 2 * K : nullptr);
}

// grid (V, splits), 256 threads.  Workgroup (v, j) takes the positions [j rps, min(R, (j + 1) rps)) of
// ids [R] and d_x [R, H], H <= 256: part [splits][V][H] at (j, v) = scale times the sum, in ascending
// position, of the rows of d_x whose id is v.  The ids are matched 256 positions at a time, one per
// thread, each wave's matches as one ballot; thread h < H then adds column h of the matching rows.
__global__ __launch_bounds__(256) void emb_dw_kernel(const int64_t* __restrict__ ids, const float* __restrict__ dx,
                                                     int R, int H, int rps, float scale, float* __restrict__ part) {
    __shared__ unsigned long long hits[2][4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t v = blockIdx.x;
    const int beg = blockIdx.y * rps, end = min(R, beg + rps);
    float acc = 0.f;
    int flip = 0;
    for (int p0 = beg; p0 < end; p0 += 256, flip ^= 1) {
        const int p = p0 + tid;
        const unsigned long long m = __ballot(p < end && ids[p] == v);
        if (lane == 0) hits[flip][wave] = m;
        __syncthreads();  // the other buffer is rewritten only after every thread has passed this barrier again
        if (tid < H)
            for (int w = 0; w < 4; ++w) {
                unsigned long long b = hits[flip][w];
                while (b) {
                    const int i = __ffsll((long long)b) - 1;
                    b &= b - 1;
                    acc += dx[(size_t)(p0 + 64 * w + i) * H + tid];
                }
            }
    }
    if (tid < H) part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * H + tid] = scale * acc;
}

// grid (cdiv(S, kLrWaves), B), 64 kLrWaves threads: wave w takes the phoneme s = kLrWaves blockIdx.x + w
// of utterance blockIdx.y.  d_enc [B, S, H] at (b, s) = the sum of d_reg [B, T_out, H] at (b, t) over
// cum[b, s] <= t < min(cum[b, s + 1], T_out), t ascending from the first frame's own value: the order
// depends on the phoneme's frame count alone.  No frames: exactly 0.  VEC: H % 4 == 0, 16-byte pieces.
template <bool VEC>
__global__ __launch_bounds__(64 * kLrWaves) void lr_adjoint_kernel(const float* __restrict__ d_reg,
                                                                   const int32_t* __restrict__ cum, int S, int H,
                                                                   int T_out, float* __restrict__ d_enc) {
    const int b = blockIdx.y, s = blockIdx.x * kLrWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= S) return;
    const int32_t* c = cum + (size_t)b * (S + 1);
    const int lo = max(c[s], 0), hi = min(c[s + 1], T_out);
    const float* src = d_reg + (size_t)b * T_out * H;
    float* dst = d_enc + ((size_t)b * S + s) * H;
    if constexpr (VEC) {
        for (int c4 = lane; c4 < H / 4; c4 += 64) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            if (lo < hi) a = *reinterpret_cast<const float4*>(src + (size_t)lo * H + 4 * c4);
#pragma unroll 4
            for (int t = lo + 1; t < hi; ++t) {
                const float4 v = *reinterpret_cast<const float4*>(src + (size_t)t * H + 4 * c4);
                a.x += v.x;
                a.y += v.y;
                a.z += v.z;
                a.w += v.w;
            }
            *reinterpret_cast<float4*>(dst + 4 * c4) = a;
        }
    } else {
        for (int h = lane; h < H; h += 64) {
            float a = lo < hi ? src[(size_t)lo * H + h] : 0.f;
#pragma unroll 4
            for (int t = lo + 1; t < hi; ++t) a += src[(size_t)t * H + h];
            dst[h] = a;
        }
    }
}

}  // namespace egrad
}  // namespace m2

namespace {
using namespace m2;
using dgrad::LaunchRow;
using dgrad::Step;
using egrad::Dims;

const char* kDimsMsg =
    "1 <= V <= 65536, H a multiple of 8 with 2 H <= 256, head_dim 16, 32, 48 or 64, layers >= 1";

// ln_bwd_kernel and the finishes of its slots; part holds ln_part_floats.
int32_t launch_ln_bwd(const float* gy, const float* x, const float* gamma, const float* g_res, size_t R, int K, float* gx,
                      float* dgamma, float* dbeta, bool add, float* part, hipStream_t st) {
    const LaunchRow r = egrad::ln_row(R, K);
    float* slots = (dgamma || dbeta) ? part : nullptr;
    const int kt = dgrad::col_tiles(K);
#define M2_LN(KTM)                                                                                                   \
    hipLaunchKernelGGL(egrad::ln_bwd_kernel<KTM>, dgrad::grid_of(r), dim3(r.threads), r.lds, st, gy, x, gamma, g_res, \
                       (int)R, K, gx, slots)
    if (kt <= 4) M2_LN(4);
    else M2_LN(8);
#undef M2_LN
    M2_LAUNCHED(r.kernel);
    return dgrad::launch_ln_finish(part, K, dgrad::dx_blocks(R), add, dgamma, dbeta, st);
}

// emb_dw_kernel and the finish; part holds emb_split's part_floats.
int32_t launch_emb_dw(const int64_t* ids, const float* dx, size_t R, int V, int H, float scale, float* d_emb, bool add,
                      float* part, hipStream_t st) {
    const egrad::EmbPlan p = egrad::emb_split(R, V, H);
    const LaunchRow r = egrad::emb_row(R, V, H);
    hipLaunchKernelGGL(egrad::emb_dw_kernel, dgrad::grid_of(r), dim3(r.threads), 0, st, ids, dx, (int)R, H, p.rps, scale,
                       part);
    M2_LAUNCHED(r.kernel);
    const size_t n = (size_t)V * H;
    return dgrad::launch_finish(part, n, p.splits, n, add, d_emb, st);
}

int32_t launch_lr_adjoint(const float* d_reg, const int32_t* cum, int B, int S, int H, int T_out, float* d_enc,
                          hipStream_t st) {
    const LaunchRow r = egrad::lr_row(B, S);
    if (H % 4 == 0)
        hipLaunchKernelGGL(egrad::lr_adjoint_kernel<true>, dgrad::grid_of(r), dim3(r.threads), 0, st, d_reg, cum, S, H,
                           T_out, d_enc);
    else
        hipLaunchKernelGGL(egrad::lr_adjoint_kernel<false>, dgrad::grid_of(r), dim3(r.threads), 0, st, d_reg, cum, S, H,
                           T_out, d_enc);
    M2_LAUNCHED(r.kernel);
    return M2_OK;
}

float embed_scale(int H) { return (float)std::sqrt((double)H); }  // the forward's hidden_dim ** 0.5

size_t tape_bytes(const Dims& d) {
    Sizer s;
    egrad::carve_tape(s, d, nullptr);
    return s.off + 256;
}

size_t backward_bytes(const Dims& d) {
    if (d.B == 0 || d.S == 0) return 256;
    Sizer s;
    egrad::carve_backward(s, d, nullptr);
    return s.off + 256;
}

constexpr int kMaxMaps = 1 + dgrad::kLayerMaps * dgrad::kMaxLayers;
}  // namespace

extern "C" {

size_t m2_encoder_tape_bytes(int32_t V, int32_t H, int32_t layers, int32_t heads, int32_t B, int32_t S) {
    const Dims d{V, H, layers, heads, B, S};
    return egrad::dims_ok(d) ? tape_bytes(d) : 0;
}

int32_t m2_encoder_tape_map(int32_t V, int32_t H, int32_t layers, int32_t heads, int32_t B, int32_t S, int32_t index,
                            size_t* offset_floats, int32_t* width) {
    const Dims d{V, H, layers, heads, B, S};
    M2_CHECK_SHAPE(egrad::dims_ok(d), kDimsMsg);
    M2_CHECK_ARG(offset_floats && width && index >= 0 && index < egrad::n_maps(d), "m2_encoder_tape_map: bad argument");
    Sizer s;  // carve_tape's arithmetic, map by map
    for (int i = 0; i <= index; ++i) {
        const size_t at = align_up(s.off, 256);
        s.take<float>(egrad::rows(d) * egrad::map_width(d, i));
        if (i == index) {
            *offset_floats = at / sizeof(float);
            *width = egrad::map_width(d, i);
        }
    }
    return M2_OK;
}

int32_t m2_encoder_train_forward(const float* const* params, int32_t V, int32_t H, int32_t layers, int32_t heads,
                                 const int64_t* ids, const float* pe, const uint8_t* key_mask, int32_t B, int32_t S,
                                 float* out, void* tape, size_t tape_bytes_, void* stream) {
    const Dims d{V, H, layers, heads, B, S};
    M2_CHECK_SHAPE(egrad::dims_ok(d), kDimsMsg);
    if (B == 0 || S == 0) return M2_OK;
    M2_CHECK_ARG(params && ids && pe && out && tape, "m2_encoder_train_forward: bad argument");
    for (int i = 0; i < egrad::n_params(d); ++i) M2_CHECK_ARG(params[i], "m2_encoder_train_forward: null parameter");
    Carve c(tape, tape_bytes_);
    float* map[kMaxMaps];
    egrad::carve_tape(c, d, map);
    if (!c.ok) return fail(M2_E_ARG, "m2_encoder_train_forward: tape too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t rc = launch_embed_pe_scaled(ids, params[0], pe, B, S, H, V, embed_scale(H), map[0], st);
    const float* cur = map[0];
    for (int l = 0; l < layers && rc == M2_OK; ++l) {
        float** m = map + egrad::map_of(l, 0);
        rc = dgrad::layer_forward(cur, params + egrad::p_layer(l, 0), m, key_mask, B, S, H, heads, st);
        cur = m[dgrad::MAP_XOUT];
    }
    if (rc != M2_OK) return rc;
    return launch_layer_norm(cur, params[egrad::p_norm(d)], params[egrad::p_norm(d) + 1], B * S, H, out, st);
}

size_t m2_encoder_backward_workspace_bytes(int32_t V, int32_t H, int32_t layers, int32_t heads, int32_t B, int32_t S) {
    const Dims d{V, H, layers, heads, B, S};
    return egrad::dims_ok(d) ? backward_bytes(d) : 0;
}

int32_t m2_encoder_backward(const float* const* params, int32_t V, int32_t H, int32_t layers, int32_t heads,
                            const int64_t* ids, const uint8_t* key_mask, int32_t B, int32_t S, const void* tape,
                            const float* d_out, float* const* grads, int32_t accumulate, void* workspace,
                            size_t workspace_bytes, void* stream) {
    const Dims d{V, H, layers, heads, B, S};
    M2_CHECK_SHAPE(egrad::dims_ok(d), kDimsMsg);
    if (B == 0 || S == 0) return M2_OK;
    M2_CHECK_ARG(params && ids && tape && d_out && grads && workspace, "m2_encoder_backward: bad argument");
    for (int i = 0; i < egrad::n_params(d); ++i) M2_CHECK_ARG(params[i], "m2_encoder_backward: null parameter");
    Sizer ts;
    egrad::carve_tape(ts, d, nullptr);
    Carve tc(const_cast<void*>(tape), ts.off);
    float* map[kMaxMaps];
    egrad::carve_tape(tc, d, map);
    Carve c(workspace, workspace_bytes);
    dgrad::Bufs bufs;
    egrad::carve_backward(c, d, &bufs);
    if (!c.ok) return fail(M2_E_ARG, "m2_encoder_backward: workspace too small");
    dgrad::Walk w{};
    w.params = params;
    w.grads = grads;
    w.maps = map;
    w.named[-dgrad::BUF_DMEL] = const_cast<float*>(d_out);
    w.named[-dgrad::BUF_DX] = grads[0] ? bufs.cot[0] : nullptr;  // the cotangent of x0: the embedding's alone
    w.named[-dgrad::BUF_COT0] = bufs.cot[0];
    w.named[-dgrad::BUF_COT1] = bufs.cot[1];
    w.named[-dgrad::BUF_WIDE] = bufs.wide;
    w.mask = key_mask;
    w.geo = egrad::geo(d);
    w.add = accumulate != 0;
    w.bufs = bufs;
    w.st = static_cast<hipStream_t>(stream);
    for (const Step& s : egrad::plan_steps(d)) {
        int32_t rc = M2_OK;
        switch (s.kind) {
            case dgrad::STEP_LN:
                rc = launch_ln_bwd(w.buf(s.gy), w.buf(s.aux), w.param(s.dgamma), nullptr, w.geo.R, s.K, w.buf(s.out),
                                   w.grad(s.dgamma), w.grad(s.dbeta), w.add, bufs.part, w.st);
                break;
            case dgrad::STEP_EMB:
                if (w.grad(s.dw))
                    rc = launch_emb_dw(ids, w.buf(s.gy), w.geo.R, V, H, embed_scale(H), w.grad(s.dw), w.add, bufs.part,
                                       w.st);
                break;
            default: rc = dgrad::run_step(s, w);
        }
        if (rc != M2_OK) return rc;
    }
    return M2_OK;
}

int32_t m2_debug_encoder_grad_plan(int32_t V, int32_t H, int32_t layers, int32_t heads, int32_t B, int32_t S, char* out,
                                   size_t cap) {
    const Dims d{V, H, layers, heads, B, S};
    M2_CHECK_ARG(out && cap > 0 && B > 0 && S > 0, "m2_debug_encoder_grad_plan: bad argument");
    M2_CHECK_SHAPE(egrad::dims_ok(d), kDimsMsg);
    const std::string line = egrad::print_plan(d);
    const size_t n = std::min(line.size(), cap - 1);
    std::memcpy(out, line.data(), n);
    out[n] = '\0';
    return (int32_t)line.size();
}

// ---- the kernels alone -------------------------------------------------------------

size_t m2_embedding_backward_workspace_bytes(int32_t R, int32_t V, int32_t H) {
    if (R <= 0 || R > (1 << 24) || !egrad::emb_ok(V, H)) return 0;
    return egrad::emb_split((size_t)R, V, H).part_floats * sizeof(float) + 256;
}

int32_t m2_embedding_backward(const int64_t* ids, const float* d_x, int32_t R, int32_t V, int32_t H, float scale,
                              float* d_emb, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(d_emb && R >= 0 && (R == 0 || (ids && d_x)), "m2_embedding_backward: bad argument");
    M2_CHECK_SHAPE(egrad::emb_ok(V, H) && R <= (1 << 24), "m2_embedding_backward: 1 <= V <= 65536, 1 <= H <= 256");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (R == 0) {  // an empty sum
        if (!accumulate) M2_HIP(hipMemsetAsync(d_emb, 0, (size_t)V * H * sizeof(float), st));
        return M2_OK;
    }
    Carve cv(workspace, workspace_bytes);
    float* part = cv.take<float>(egrad::emb_split((size_t)R, V, H).part_floats);
    if (!cv.ok) return fail(M2_E_ARG, "m2_embedding_backward: workspace too small");
    return launch_emb_dw(ids, d_x, (size_t)R, V, H, scale, d_emb, accumulate != 0, part, st);
}

size_t m2_layer_norm_backward_workspace_bytes(int32_t R, int32_t K) {
    if (R <= 0 || R > (1 << 24) || !egrad::ln_ok(K)) return 0;
    return egrad::ln_part_floats((size_t)R, K) * sizeof(float) + 256;
}

int32_t m2_layer_norm_backward(const float* g_y, const float* x, const float* gamma, const float* g_res, int32_t R,
                               int32_t K, float* g_x, float* dgamma, float* dbeta, void* workspace,
                               size_t workspace_bytes, void* stream) {
    M2_CHECK_ARG(R >= 0 && (g_x || dgamma || dbeta) && (R == 0 || (g_y && x && gamma)),
                 "m2_layer_norm_backward: bad argument");
    M2_CHECK_SHAPE(egrad::ln_ok(K) && R <= (1 << 24), "m2_layer_norm_backward: K a multiple of 8, at most 128");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (R == 0) {  // empty sums
        if (dgamma) M2_HIP(hipMemsetAsync(dgamma, 0, (size_t)K * sizeof(float), st));
        if (dbeta) M2_HIP(hipMemsetAsync(dbeta, 0, (size_t)K * sizeof(float), st));
        return M2_OK;
    }
    float* part = nullptr;
    if (dgamma || dbeta) {
        Carve cv(workspace, workspace_bytes);
        part = cv.take<float>(egrad::ln_part_floats((size_t)R, K));
        if (!cv.ok) return fail(M2_E_ARG, "m2_layer_norm_backward: workspace too small");
    }
    return launch_ln_bwd(g_y, x, gamma, g_res, (size_t)R, K, g_x, dgamma, dbeta, false, part, st);
}

int32_t m2_length_regulator_backward(const float* d_reg, const int32_t* cum, int32_t B, int32_t S, int32_t H,
                                     int32_t T_out, float* d_enc, void* stream) {
    M2_CHECK_ARG(B >= 0 && S >= 0 && H > 0 && T_out >= 0, "m2_length_regulator_backward: bad argument");
    M2_CHECK_SHAPE(B <= loss::kMaxGrid, "m2_length_regulator_backward: too many utterances");
    if (B == 0 || S == 0) return M2_OK;
    M2_CHECK_ARG(cum && d_enc && (d_reg || T_out == 0), "m2_length_regulator_backward: bad argument");
    return launch_lr_adjoint(d_reg, cum, B, S, H, T_out, d_enc, static_cast<hipStream_t>(stream));
}

}  // extern "C"
