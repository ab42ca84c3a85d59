// The training side of DurationPredictor: a forward that keeps a tape, from the 10 raw parameters (no
// model handle) and the eval-mode BatchNorm constants, and the gradient with respect to those parameters
// and the encoder output.  Exact f32, no floating-point atomics: every reduction runs in a fixed order,
// so equal inputs give equal bits (decoder_grad.hip's rules); d_enc has no reduction over the batch.
//
//   forward   the per-op path of a stand-alone DurationPredictor: launch_conv of vocoder.hip with the
//             affine, ReLU and (conv1) the transposed read of enc, each block writing its map into the
//             tape, then the k = 1 projection with softplus.
//   backward  duration_grad_plan.h's plan_steps() in order.  The convs' data, weight and bias gradients
//             through losses.hip's launchers (conv_launch.h) on the exact-f32 MFMA; u through the
//             forward's own conv launch; the kernels here, bound by their loads and stores (plain fmaf):
//             dur_bn_bwd_kernel     one workgroup per (utterance, 64 positions), a lane per position,
//                                   a wave per channel: BatchNorm's and ReLU's backward with the slots of
//                                   d gamma and d beta; as the head it first forms g_z from d_dur and the
//                                   recomputed z, and adds the slots of d pw and d pb: g_z and g_y2 never
//                                   reach memory.
//             dur_transpose_kernel  [B, R, C] -> [B, C, R] through a 32 x 32 tile at a pitch of 33 floats
//                                   (conflict-free under the 32-bank rule of 4-byte LDS accesses both
//                                   ways), 16-byte stores when R % 4 == 0.
#include <algorithm>
#include <cstring>

#include "conv_launch.h"
#include "duration_grad_plan.h"

namespace m2 {

namespace dgrad {
// decoder_grad.hip: dst = (add ? dst : 0) + the sum over `slots` partials of n floats, `stride` apart.
int32_t launch_finish(const float* part, size_t n, int slots, size_t stride, bool add, float* dst, hipStream_t st);
}  // namespace dgrad

namespace dugrad {

__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// grid (cdiv(S, kChunk), B), 256 threads; HEAD: H kChunk floats of LDS.  y [B, H, S] is the block's
// post-ReLU output, u (or null: no d gamma) its conv output with the bias, alpha, mean, invstd [H] the
// block's BatchNorm constants.  Lane l takes the position p = kChunk blockIdx.x + l, wave w the channels
// w, w + 4, ...  The cotangent of y at (c, p) is g_in [B, H, S] or, as the head, pw[c] g_z[p] with
//   z[p] = (fmaf over c ascending of pw[c] y[c][p]) + pb,   g_z = d_dur (z > 20 ? 1 : sigmoid(z)),
// g_in then being d_dur [B, S].  g_a = g_y [y > 0]; gu [B, H, S] = g_a alpha[c].  The workgroup's slot
// (slots [B gridDim.x][stride], utterance-major) receives the sums over its positions, each a wave's
// xor-shuffle tree: d gamma[c] = sum g_a (u - mean[c]) invstd[c] at [c] (when u is given), d beta[c] =
// sum g_a at [H + c] and, as the head, d pw[c] = sum g_z y at [2 H + c] and d pb = sum g_z at [3 H].
template <bool HEAD>
__global__ __launch_bounds__(256) void dur_bn_bwd_kernel(const float* __restrict__ g_in, const float* __restrict__ y,
                                                         const float* __restrict__ u, const float* __restrict__ pw,
                                                         const float* __restrict__ pb, const float* __restrict__ alpha,
                                                         const float* __restrict__ mean,
                                                         const float* __restrict__ invstd, int H, int S,
                                                         float* __restrict__ gu, float* __restrict__ slots, int stride) {
    extern __shared__ float ys[];  // HEAD: [H][kChunk]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = blockIdx.y, p = blockIdx.x * kChunk + lane;
    const bool in = p < S;
    const size_t base = (size_t)b * H * S;
    float gz = 0.f;
    if constexpr (HEAD) {
        for (int c = wave; c < H; c += 4) ys[c * kChunk + lane] = in ? y[base + (size_t)c * S + p] : 0.f;
        __syncthreads();
        float acc = 0.f;
        for (int c = 0; c < H; ++c) acc = fmaf(pw[c], ys[c * kChunk + lane], acc);
        const float z = acc + pb[0];
        if (in) gz = g_in[(size_t)b * S + p] * (z > 20.f ? 1.f : 1.f / (1.f + expf(-z)));
    }
    float* slot = slots + ((size_t)b * gridDim.x + blockIdx.x) * stride;
    for (int c = wave; c < H; c += 4) {
        const size_t i = base + (size_t)c * S + p;
        float yv, gy;
        if constexpr (HEAD) {
            yv = ys[c * kChunk + lane];
            gy = pw[c] * gz;
        } else {
            yv = in ? y[i] : 0.f;
            gy = in ? g_in[i] : 0.f;
        }
        const float ga = yv > 0.f ? gy : 0.f;
        if (in) gu[i] = ga * alpha[c];
        if (u != nullptr) {  // the same for every thread of the workgroup
            const float sg = wave_sum(in ? ga * ((u[i] - mean[c]) * invstd[c]) : 0.f);
            if (lane == 0) slot[c] = sg;
        }
        const float sb = wave_sum(ga);
        if (lane == 0) slot[H + c] = sb;
        if constexpr (HEAD) {
            const float sw = wave_sum(gz * yv);
            if (lane == 0) slot[2 * H + c] = sw;
        }
    }
    if constexpr (HEAD) {
        if (wave == 0) {
            const float s = wave_sum(gz);
            if (lane == 0) slot[3 * H] = s;
        }
    }
}

// grid (cdiv(C, kTile), cdiv(R, kTile), B), 256 threads.  in [B, R, C] -> out [B, C, R].  The tile is
// loaded along C (32 consecutive floats per row) and stored along R.  VEC: R % 4 == 0 and out 16-byte
// aligned; a thread then stores the four rows 4 q .. 4 q + 3 of one column as one 16-byte piece.
template <bool VEC>
__global__ __launch_bounds__(256) void dur_transpose_kernel(const float* __restrict__ in, int R, int C,
                                                            float* __restrict__ out) {
    __shared__ float tile[kTile][kTile + 1];
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const int r0 = blockIdx.y * kTile, c0 = blockIdx.x * kTile;
    const size_t base = (size_t)blockIdx.z * R * C;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = r0 + ty + 8 * j, c = c0 + tx;
        tile[ty + 8 * j][tx] = (r < R && c < C) ? in[base + (size_t)r * C + c] : 0.f;
    }
    __syncthreads();
    if constexpr (VEC) {
        const int q = tid & 7, cl = tid >> 3;
        const int c = c0 + cl, r = r0 + 4 * q;
        if (c < C && r < R)
            *reinterpret_cast<float4*>(out + base + (size_t)c * R + r) =
                make_float4(tile[4 * q][cl], tile[4 * q + 1][cl], tile[4 * q + 2][cl], tile[4 * q + 3][cl]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + ty + 8 * j, r = r0 + tx;
            if (c < C && r < R) out[base + (size_t)c * R + r] = tile[tx][ty + 8 * j];
        }
    }
}

}  // namespace dugrad
}  // namespace m2

namespace {
using namespace m2;
using dugrad::Dims;
using dugrad::LaunchRow;
using dugrad::Step;

const char* kDimsMsg = "kernel size 3, H a multiple of 8 from 16 to 128, at most 2^20 positions per utterance";

dim3 grid_of(const LaunchRow& r) { return dim3(r.gx, r.gy, r.gz); }

// dur_bn_bwd_kernel; the slots are finished by the caller.
int32_t launch_bn_bwd(bool head, const float* g_in, const float* y, const float* u, const float* pw, const float* pb,
                      const float* bn, const Dims& d, float* gu, float* slots, hipStream_t st) {
    const LaunchRow r = dugrad::bn_row(d, head);
    const int stride = (int)dugrad::slot_floats(d.H, head);
    const float *alpha = bn + dugrad::BN_ALPHA * d.H, *mean = bn + dugrad::BN_MEAN * d.H,
                *invstd = bn + dugrad::BN_INVSTD * d.H;
    if (head)
        hipLaunchKernelGGL(dugrad::dur_bn_bwd_kernel<true>, grid_of(r), dim3(r.threads), r.lds, st, g_in, y, u, pw, pb,
                           alpha, mean, invstd, d.H, d.S, gu, slots, stride);
    else
        hipLaunchKernelGGL(dugrad::dur_bn_bwd_kernel<false>, grid_of(r), dim3(r.threads), r.lds, st, g_in, y, u, pw, pb,
                           alpha, mean, invstd, d.H, d.S, gu, slots, stride);
    M2_LAUNCHED(r.kernel);
    return M2_OK;
}

// in [B, R, C] -> out [B, C, R]
int32_t launch_transpose(const float* in, int B, int R, int C, float* out, hipStream_t st) {
    const LaunchRow r = dugrad::tr_row(B, R, C);
    if (R % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0)
        hipLaunchKernelGGL(dugrad::dur_transpose_kernel<true>, grid_of(r), dim3(r.threads), 0, st, in, R, C, out);
    else
        hipLaunchKernelGGL(dugrad::dur_transpose_kernel<false>, grid_of(r), dim3(r.threads), 0, st, in, R, C, out);
    M2_LAUNCHED(r.kernel);
    return M2_OK;
}

size_t tape_bytes(const Dims& d) {
    Sizer s;
    dugrad::carve_tape(s, d, nullptr);
    return s.off + 256;
}

size_t backward_bytes(const Dims& d) {
    if (d.B == 0 || d.S == 0) return 256;
    Sizer s;
    dugrad::carve_backward(s, d, nullptr);
    return s.off + 256;
}
}  // namespace

extern "C" {

size_t m2_duration_tape_bytes(int32_t H, int32_t B, int32_t S) {
    const Dims d{H, B, S};
    return dugrad::dims_ok(d) ? tape_bytes(d) : 0;
}

int32_t m2_duration_tape_map(int32_t H, int32_t B, int32_t S, int32_t index, size_t* offset_floats, int32_t* width) {
    const Dims d{H, B, S};
    M2_CHECK_SHAPE(dugrad::dims_ok(d), kDimsMsg);
    M2_CHECK_ARG(offset_floats && width && index >= 0 && index < dugrad::kMaps, "m2_duration_tape_map: bad argument");
    Sizer s;  // carve_tape's arithmetic, map by map
    for (int i = 0; i <= index; ++i) {
        const size_t at = align_up(s.off, 256);
        s.take<float>(dugrad::map_floats(d));
        if (i == index) {
            *offset_floats = at / sizeof(float);
            *width = H;
        }
    }
    return M2_OK;
}

int32_t m2_duration_train_forward(const float* const* params, const float* bn, int32_t H, const float* enc, int32_t B,
                                  int32_t S, float* dur, void* tape, size_t tape_bytes_, void* stream) {
    const Dims d{H, B, S};
    M2_CHECK_SHAPE(dugrad::dims_ok(d), kDimsMsg);
    if (B == 0 || S == 0) return M2_OK;
    M2_CHECK_ARG(params && bn && enc && dur && tape, "m2_duration_train_forward: bad argument");
    for (int i = 0; i < dugrad::kParams; ++i) M2_CHECK_ARG(params[i], "m2_duration_train_forward: null parameter");
    Carve c(tape, tape_bytes_);
    float* map[dugrad::kMaps];
    dugrad::carve_tape(c, d, map);
    if (!c.ok) return fail(M2_E_ARG, "m2_duration_train_forward: tape too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float *bn1 = bn, *bn2 = bn + 4 * (size_t)H;
    int32_t rc = launch_conv(enc, params[dugrad::P_W1], params[dugrad::P_B1], bn1 + dugrad::BN_ALPHA * H,
                             bn1 + dugrad::BN_BETA * H, nullptr, 3, ACT_RELU, true, B, H, H, S, map[dugrad::MAP_Y1], st);
    if (rc != M2_OK) return rc;
    rc = launch_conv(map[dugrad::MAP_Y1], params[dugrad::P_W2], params[dugrad::P_B2], bn2 + dugrad::BN_ALPHA * H,
                     bn2 + dugrad::BN_BETA * H, nullptr, 3, ACT_RELU, false, B, H, H, S, map[dugrad::MAP_Y2], st);
    if (rc != M2_OK) return rc;
    return launch_conv(map[dugrad::MAP_Y2], params[dugrad::P_PW], params[dugrad::P_PB], nullptr, nullptr, nullptr, 1,
                       ACT_SOFTPLUS, false, B, H, 1, S, dur, st);
}

size_t m2_duration_backward_workspace_bytes(int32_t H, int32_t B, int32_t S) {
    const Dims d{H, B, S};
    return dugrad::dims_ok(d) ? backward_bytes(d) : 0;
}

int32_t m2_duration_backward(const float* const* params, const float* bn, int32_t H, const float* enc, int32_t B,
                             int32_t S, const void* tape, const float* d_dur, float* d_enc, float* const* grads,
                             int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    const Dims d{H, B, S};
    M2_CHECK_SHAPE(dugrad::dims_ok(d), kDimsMsg);
    if (B == 0 || S == 0) return M2_OK;
    M2_CHECK_ARG(params && bn && enc && tape && d_dur && grads && workspace, "m2_duration_backward: bad argument");
    for (int i = 0; i < dugrad::kParams; ++i) M2_CHECK_ARG(params[i], "m2_duration_backward: null parameter");
    Sizer ts;
    dugrad::carve_tape(ts, d, nullptr);
    Carve tc(const_cast<void*>(tape), ts.off);
    float* map[dugrad::kMaps];
    dugrad::carve_tape(tc, d, map);
    Carve c(workspace, workspace_bytes);
    dugrad::Bufs bufs;
    dugrad::carve_backward(c, d, &bufs);
    if (!c.ok) return fail(M2_E_ARG, "m2_duration_backward: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool add = accumulate != 0;
    const loss::ConvGeo g = dugrad::geo(d);
    const int nslots = (int)dugrad::slots(d);
    const size_t nw = (size_t)3 * H * H;
    // what block 1 and the transposes are needed for
    const bool any1 = grads[dugrad::P_W1] || grads[dugrad::P_B1] || grads[dugrad::P_G1] || grads[dugrad::P_BE1];
    const bool below2 = d_enc || any1;  // whether conv2's data gradient is read
    for (const Step& s : dugrad::plan_steps(d)) {
        const int p0 = 4 * s.block;  // the block's conv.weight; + 1 conv.bias, + 2 norm.weight, + 3 norm.bias
        const float* bnb = bn + 4 * (size_t)H * std::max(s.block, 0);
        int32_t rc = M2_OK;
        switch (s.kind) {
            case dugrad::STEP_XT:
                if (below2) rc = launch_transpose(enc, B, S, H, bufs.xt, st);
                break;
            case dugrad::STEP_U:
                if (grads[p0 + 2])
                    rc = launch_conv(s.block ? map[dugrad::MAP_Y1] : bufs.xt, params[p0], params[p0 + 1], nullptr,
                                     nullptr, nullptr, 3, ACT_NONE, false, B, H, H, S, bufs.u, st);
                break;
            case dugrad::STEP_HEAD: {
                const size_t stride = dugrad::slot_floats(H, true);
                rc = launch_bn_bwd(true, d_dur, map[dugrad::MAP_Y2], grads[dugrad::P_G2] ? bufs.u : nullptr,
                                   params[dugrad::P_PW], params[dugrad::P_PB], bnb, d, bufs.gu, bufs.part, st);
                float* const dst[4] = {grads[dugrad::P_G2], grads[dugrad::P_BE2], grads[dugrad::P_PW],
                                       grads[dugrad::P_PB]};
                for (int i = 0; i < 4 && rc == M2_OK; ++i)
                    if (dst[i])
                        rc = dgrad::launch_finish(bufs.part + (size_t)i * H, i < 3 ? (size_t)H : 1, nslots, stride, add,
                                                  dst[i], st);
                break;
            }
            case dugrad::STEP_BN: {
                if (!below2) break;
                const size_t stride = dugrad::slot_floats(H, false);
                rc = launch_bn_bwd(false, bufs.gy, map[dugrad::MAP_Y1], grads[dugrad::P_G1] ? bufs.u : nullptr, nullptr,
                                   nullptr, bnb, d, bufs.gu, bufs.part, st);
                float* const dst[2] = {grads[dugrad::P_G1], grads[dugrad::P_BE1]};
                for (int i = 0; i < 2 && rc == M2_OK; ++i)
                    if (dst[i]) rc = dgrad::launch_finish(bufs.part + (size_t)i * H, (size_t)H, nslots, stride, add, dst[i], st);
                break;
            }
            case dugrad::STEP_CONV: {
                float *const dw_out = grads[p0], *const db_out = grads[p0 + 1];
                const bool dx = s.block ? below2 : d_enc != nullptr;
                if (!dx && !dw_out && !db_out) break;
                // with `accumulate` the gradient is formed in the workspace as without it, then added
                float* dw = dw_out && add ? bufs.wtmp : dw_out;
                float* db = db_out && add ? bufs.btmp : db_out;
                rc = loss::launch_conv_bwd(s.block ? map[dugrad::MAP_Y1] : bufs.xt, params[p0], bufs.gu, g, B, S, false,
                                           1.f, dx ? bufs.gy : nullptr, dw, db, false, bufs.part, st);
                if (rc == M2_OK && add && dw_out) rc = dgrad::launch_finish(bufs.wtmp, nw, 1, nw, true, dw_out, st);
                if (rc == M2_OK && add && db_out) rc = dgrad::launch_finish(bufs.btmp, (size_t)H, 1, (size_t)H, true, db_out, st);
                break;
            }
            case dugrad::STEP_DT:
                if (d_enc) rc = launch_transpose(bufs.gy, B, H, S, d_enc, st);
                break;
        }
        if (rc != M2_OK) return rc;
    }
    return M2_OK;
}

int32_t m2_debug_duration_grad_plan(int32_t H, int32_t B, int32_t S, char* out, size_t cap) {
    const Dims d{H, B, S};
    M2_CHECK_ARG(out && cap > 0 && B > 0 && S > 0, "m2_debug_duration_grad_plan: bad argument");
    M2_CHECK_SHAPE(dugrad::dims_ok(d), kDimsMsg);
    const std::string line = dugrad::print_plan(d);
    const size_t n = std::min(line.size(), cap - 1);
    std::memcpy(out, line.data(), n);
    out[n] = '\0';
    return (int32_t)line.size();
}

}  // extern "C"
