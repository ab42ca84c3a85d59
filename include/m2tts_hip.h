/*
 * m2tts_hip.h - C ABI of the MI355X (gfx950) implementation of the m2-tts
 * mel-synthesis + vocoder forward path.
 *
 * The reference (Ryannasr11/m2-tts) has no FFI layer: its boundary is the
 * Python nn.Module API of src/models/tts_model.py and components.py.  Each
 * entry point below replaces the PyTorch op sequence of one reference
 * module's forward; the citation is given per function.  The Python drop-in
 * (m2-tts_amd/src/models/) binds these with ctypes - see INTEGRATION.md.
 *
 * Conventions
 *  - All tensors are caller-owned DEVICE pointers (torch tensor.data_ptr()),
 *    contiguous, fp32 unless stated; ids/lengths are int64.
 *  - `stream` is a hipStream_t passed as void* (torch current stream's
 *    cuda_stream); every call is stream-ordered and asynchronous.  No call
 *    allocates or synchronises, except m2_model_create (one-time weight
 *    packing) and m2_model_destroy.
 *  - Scratch memory is the caller's: size it with m2_workspace_bytes().
 *  - Return 0 on success; M2_E_* (<0) for argument/shape errors; a positive
 *    value is a hipError_t passed through.  m2_last_error() returns a
 *    thread-local message for the last failure on the calling thread.
 *  - One stream per model handle: a model's calls must be ordered on one
 *    stream (or externally synchronised).  The handle carries per-model
 *    device state that successive calls hand over in stream order - the
 *    split-f16 range flag (m2_model_check) and the work-queue counters of the
 *    one-launch transformer layers - so two streams using one handle at the
 *    same time may see each other's range flag and must not share it; create
 *    one handle per stream instead (weights are packed per handle).
 */
#ifndef M2TTS_HIP_H
#define M2TTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M2_ABI_VERSION 1

#define M2_OK 0
#define M2_E_ARG (-1)         /* null pointer / bad enum / bad size           */
#define M2_E_SHAPE (-2)       /* shape outside what the kernels support       */
#define M2_E_WORKSPACE (-3)   /* workspace smaller than m2_workspace_bytes()  */
#define M2_E_WEIGHTS (-4)     /* weight table incomplete                      */
#define M2_E_INTERNAL (-5)    /* internal protocol failure (see m2_last_error) */
#define M2_E_RANGE (-6)       /* an earlier vocoder call on this model produced non-finite audio
                                 on the split-f16 path (input or activation outside its range);
                                 see m2_model_check / m2_set_range_policy                        */

/* M2TTSModel.__init__ hyper-parameters (tts_model.py:303-313), plus the
 * positional-encoding table length (TextEncoder max_seq_len, tts_model.py:29). */
typedef struct m2_config {
    int32_t vocab_size;          /* 256 */
    int32_t hidden_dim;          /* H: 64 stage1, 96 stage2 */
    int32_t mel_channels;        /* M: 64 / 80 */
    int32_t text_encoder_layers; /* 2 / 3 */
    int32_t decoder_layers;      /* 2 / 3 */
    int32_t num_heads;           /* 2 */
    int32_t vocoder_channels;    /* C: 128 / 256 */
    int32_t max_positions;       /* 1000 */
} m2_config;

typedef struct m2_model m2_model;

int32_t m2_abi_version(void);
const char* m2_last_error(void);

/* ---- weight table ---------------------------------------------------------
 * The weights are addressed by their reference state_dict key
 * (M2TTSModel.state_dict(), tts_model.py:303-343).  m2_weight_count/name/numel
 * enumerate the keys in the order m2_model_create expects. */
int32_t m2_weight_count(const m2_config* cfg);
int32_t m2_weight_name(const m2_config* cfg, int32_t index, char* buf, int32_t buflen);
int64_t m2_weight_numel(const m2_config* cfg, int32_t index);

/* Packs and uploads the weights once (BatchNorm folded into the duration
 * convs, conv weights re-laid out for the kernels).  `weights[i]` is a device
 * pointer to the tensor named by m2_weight_name(cfg, i) (fp32; the BatchNorm
 * num_batches_tracked entries are int64 and ignored).  Reads the weights back
 * to the host once and synchronises `stream`. */
int32_t m2_model_create(const m2_config* cfg, const void* const* weights, int32_t n_weights,
                        void* stream, m2_model** out);
int32_t m2_model_destroy(m2_model* model);

/* Re-reads the developer switches (M2_* environment variables that force one
 * code path for A/B comparisons and tests) into the library's switch table.
 * The table is read when the library loads and at every m2_model_create;
 * no entry point reads the environment per call.  Not part of the
 * reference's surface (it has no FFI). */
void m2_reload_switches(void);
int32_t m2_model_config(const m2_model* model, m2_config* out);

/* Scratch bytes needed by the stage calls for a batch of B utterances of S
 * phonemes and T mel frames (T = 0: encoder/duration only). */
size_t m2_workspace_bytes(const m2_model* model, int32_t B, int32_t S, int32_t T);

/* ---- stage entry points ---------------------------------------------------*/

/* TextEncoder.forward (tts_model.py:57-89): embedding*sqrt(H) + pe, L_enc pre-LN
 * transformer layers with key-padding mask (components.py:131-140, 59-90,
 * 226-241), final LayerNorm.  lengths may be NULL (no mask).
 * out_enc [B,S,H]; out_mask [B,S] uint8 (may be NULL). */
int32_t m2_text_encoder(const m2_model* model, const int64_t* ids, const int64_t* lengths,
                        int32_t B, int32_t S, float* out_enc, uint8_t* out_mask,
                        void* workspace, size_t workspace_bytes, void* stream);

/* DurationPredictor.forward (tts_model.py:99-117): 2x[Conv1d k3 + BN(eval) +
 * ReLU] -> Conv1d k1 -> softplus.  enc [B,S,H] -> out_dur [B,S]. */
int32_t m2_duration_predictor(const m2_model* model, const float* enc, int32_t B, int32_t S,
                              float* out_dur, void* workspace, size_t workspace_bytes, void* stream);

/* LengthRegulator.forward, counting half (tts_model.py:146-162): per phoneme
 * n = int(trunc(dur*scale)) (fp32 product, truncation toward zero, n<=0 -> 0);
 * per utterance exclusive prefix sums out_cum [B,S+1] (int32), totals
 * out_T [B] and the batch maximum out_Tmax [1] (int32).  `dur` is fp32, or
 * int32 when dur_is_int != 0 (scale then ignored). */
int32_t m2_length_regulator_count(const void* dur, int32_t dur_is_int, float scale,
                                  int32_t B, int32_t S, int32_t* out_cum, int32_t* out_T,
                                  int32_t* out_Tmax, void* stream);

/* m2_length_regulator_count, plus the one host read the regulator needs
 * (tts_model.py:163-166: the batch maximum sizes the output): also stores
 * T_max into *host_Tmax (host memory) before returning, by a mailbox the
 * count kernel posts to coherent host-mapped memory, polled by this call -
 * in place of a device->host copy and a stream synchronisation.  Blocks the
 * calling thread until the work queued on `stream` before it and the count
 * kernel are done.  One calling thread per device. */
int32_t m2_length_regulator_count_sync(const void* dur, int32_t dur_is_int, float scale,
                                       int32_t B, int32_t S, int32_t* out_cum, int32_t* out_T,
                                       int32_t* out_Tmax, int32_t* host_Tmax, void* stream);

/* LengthRegulator.forward, expanding half (tts_model.py:146-178): frame t of
 * utterance b copies enc[b, s] for cum[b,s] <= t < cum[b,s+1]; frames past
 * the utterance's total are zero; the output has exactly T_out frames
 * (padding or truncation, tts_model.py:165-176).  out [B,T_out,H]. */
int32_t m2_length_regulator_expand(const float* enc, const int32_t* cum, int32_t B, int32_t S,
                                   int32_t H, int32_t T_out, float* out, void* stream);

/* MelDecoder.forward (tts_model.py:211-228): L_dec pre-LN transformer layers
 * WITHOUT mask over the frames, LayerNorm, Linear(H->M).
 * x [B,T,H] -> out_mel [B,T,M].  x is not modified. */
int32_t m2_mel_decoder(const m2_model* model, const float* x, int32_t B, int32_t T, float* out_mel,
                       void* workspace, size_t workspace_bytes, void* stream);

/* SimpleVocoder.forward (tts_model.py:279-297): input_conv, 4x[ConvT(k=2r,s=r,
 * p=r/2) + leaky(0.1) + LightweightResBlock], output_conv + tanh.
 * mel_layout 0: mel [B,M,T] (the module's own input); 1: mel [B,T,M] (the
 * decoder output, read transposed in place).  out_audio [B,1,64T]. */
int32_t m2_vocoder(const m2_model* model, const float* mel, int32_t mel_layout, int32_t B,
                   int32_t T, float* out_audio, void* workspace, size_t workspace_bytes,
                   void* stream);

/* ---- streamed / chunked vocoder (long-form; SURVEY 8b `chunk_frames`) ------
 * The reference runs SimpleVocoder over the whole mel (tts_model.py:279-297).
 * A chunk [f0, f1) of mel frames is computed over the window
 * [f0 - halo, f1 + halo) clipped to [0, T), halo = m2_vocoder_halo_frames()
 * = the vocoder's receptive field (3 frames per side), so every audio sample
 * equals the whole-utterance call's bit for bit; the window's mel is copied to
 * the workspace, vocoded, and the centre of its audio copied out.
 *   m2_vocoder_set_chunking: m2_vocoder (and m2_inference / _back) then run
 *     chunk_frames frames at a time (0 = whole utterance, the default); size
 *     the workspace after changing it (m2_workspace_bytes depends on it).
 *   m2_vocoder_chunk: audio of frames [f0, f1) only, out_chunk [B,1,64(f1-f0)]
 *     (for streaming: chunk k can be played while chunk k+1 is computed);
 *     workspace from m2_vocoder_chunk_workspace_bytes(B, T, f1 - f0). */
int32_t m2_vocoder_set_chunking(m2_model* model, int32_t chunk_frames);
int32_t m2_vocoder_halo_frames(void);
int32_t m2_vocoder_chunk(const m2_model* model, const float* mel, int32_t mel_layout, int32_t B,
                         int32_t T, int32_t f0, int32_t f1, float* out_chunk, void* workspace,
                         size_t workspace_bytes, void* stream);
size_t m2_vocoder_chunk_workspace_bytes(const m2_model* model, int32_t B, int32_t T,
                                        int32_t chunk_frames);

/* ---- range of the split-f16 arithmetic -------------------------------------
 * The split path carries fp32 values as f16 hi/lo pairs; a value of magnitude
 * >= 65520 (input mel or any activation) becomes hi = inf, lo = NaN, and the
 * NaN reaches the audio, whose last kernel raises a per-model flag (never a
 * silently wrong finite result).  Transformer activations are bounded by the
 * LayerNorm weights and checked once at m2_model_create (out of range -> the
 * exact-f32 transformer kernels).  What a raised flag does:
 *   policy 0 (report, default): asynchronous, like a HIP kernel error - the
 *     next m2_vocoder / m2_inference* call on the model returns M2_E_RANGE
 *     (and clears the flag); m2_model_check synchronises `stream` and
 *     reports it at once (*flagged = 1, flag cleared).
 *   policy 1 (fallback): the non-finite part of the call is recomputed in
 *     fp32 on the device, without a host wait.  On the pipelined tails (the
 *     stage1 / stage2 split-f16 defaults) each workgroup whose strip stored a
 *     non-finite sample recomputes only that strip's frames inside the tail
 *     launch by direct fp32 convolution in the reference's layer order
 *     (csrc/vocoder_redo.h): the reference's op sequence in fp32, in another
 *     summation order than the exact-f32 kernels, so within the
 *     reference-conditioned tolerance of tests/test_gpu_range.py, NOT
 *     bit-equal to them; non-finite only if the reference's result is.
 *     M2_REDO_LAUNCH=1 (and the windowed x3 tails) instead enqueue the
 *     guarded exact-f32 launch behind the split kernels (it returns at once
 *     unless their device flag word is raised; two words alternate between
 *     calls, the next call's first kernel zeroes the other), whose output is
 *     bit-equal to the exact-f32 kernels.  Other shapes: m2_vocoder
 *     synchronises `stream` and re-runs the call on the exact-f32 kernels. */
int32_t m2_set_range_policy(m2_model* model, int32_t policy);
int32_t m2_model_check(m2_model* model, void* stream, int32_t* flagged);

/* Select the vocoder arithmetic at run time: 1 = exact-f32 MFMA kernels,
 * 2 = split-f16 MFMA kernels (the default when the model has their packs).
 * M2_E_ARG when the model has no packs for the requested path. */
int32_t m2_vocoder_select(m2_model* model, int32_t path);

/* ---- whole-inference entry points (M2TTSModel.inference, tts_model.py:402-438)
 * Two calls split at the one host read the path needs (T_max sizes the
 * outputs), so a step costs two host->library crossings instead of six:
 *   m2_inference_front: text encoder (+ padding mask when lengths != NULL),
 *     duration predictor, frame counts; blocks until T_max is posted
 *     (as m2_length_regulator_count_sync) and stores it in *host_Tmax.
 *   m2_inference_back: length-regulator expansion to T frames (the caller
 *     passes max(1, T_max), tts_model.py:158-160), mel decoder, vocoder.
 *     out_mel [B,T,M], out_audio [B,1,64T].
 * `front` (m2_front_bytes(B,S)) carries the encoder output, durations and
 * frame counts from the first call to the second; `workspace` is sized by
 * m2_inference_workspace_bytes(B,S,T) (T = 0 for the front call). */
size_t m2_front_bytes(const m2_model* model, int32_t B, int32_t S);
size_t m2_inference_workspace_bytes(const m2_model* model, int32_t B, int32_t S, int32_t T);
int32_t m2_inference_front(const m2_model* model, const int64_t* ids, const int64_t* lengths,
                           int32_t B, int32_t S, float scale, void* front, size_t front_bytes,
                           void* workspace, size_t workspace_bytes, int32_t* host_Tmax,
                           void* stream);
int32_t m2_inference_back(const m2_model* model, int32_t B, int32_t S, int32_t T,
                          const void* front, size_t front_bytes, float* out_mel,
                          float* out_audio, void* workspace, size_t workspace_bytes,
                          void* stream);

/* Both halves in ONE call when the outputs fit.  The buffers give a frame
 * capacity T_cap = min(mel_cap / (B*M), audio_cap / (B*64)) (if the workspace
 * holds m2_inference_workspace_bytes(B,S,T_cap)); with one, and when
 * m2_inference_dev_supported(model, T_cap), the back half is enqueued right
 * behind the count kernel BEFORE the host reads T_max, its grids sized for
 * T_cap and its kernels taking T = max(1, T_max) from the device (the host
 * wait then overlaps the decoder instead of idling the GPU); otherwise it is
 * enqueued after the read, if B*T*M / B*64*T fit.  The outputs are written
 * contiguously from the start of the buffers ([B,T,M] and [B,1,64T]) and
 * *launched = 1.  When T exceeds the capacity (the speculative launches then
 * did nothing) *launched = 0 and the caller allocates for *host_T and calls
 * m2_inference_back (the front buffer holds the hand-off).
 * M2_SPECULATIVE=0 in the environment turns the device-side frame count off. */
int32_t m2_inference(const m2_model* model, const int64_t* ids, const int64_t* lengths, int32_t B,
                     int32_t S, float scale, void* front, size_t front_bytes, void* workspace,
                     size_t workspace_bytes, float* mel_buf, size_t mel_cap, float* audio_buf,
                     size_t audio_cap, int32_t* host_T, int32_t* launched, void* stream);

/* Device-side frame count for sharded inference (no host read between the
 * halves): m2_inference_front_dev writes this shard's T_max to the device word
 * dev_Tmax (e.g. the payload of the ranks' all-reduce(MAX)) without waiting;
 * m2_inference_back_dev launches the back half for a capacity of T_cap frames
 * and takes T = max(1, *dev_T) from the device; when T > T_cap it does
 * nothing (the caller reads T and runs m2_inference_back).  Outputs as
 * m2_inference's.  m2_inference_dev_supported: 1 when this model's back half
 * can run so at T_cap (one-launch decoder layers with the fused mel
 * projection, the fused unchunked vocoder).  The back half's first launch
 * posts T = max(1, *dev_T) (also when it exceeds T_cap) to a host-mapped word
 * of the model: m2_frames_wait blocks until the post of the model's latest
 * m2_inference_back_dev call is visible and returns that T (no stream
 * synchronisation, no copy: the back half keeps running). */
int32_t m2_inference_dev_supported(const m2_model* model, int32_t T_cap);
int32_t m2_inference_front_dev(const m2_model* model, const int64_t* ids, const int64_t* lengths,
                               int32_t B, int32_t S, float scale, void* front, size_t front_bytes,
                               void* workspace, size_t workspace_bytes, int32_t* dev_Tmax, void* stream);
int32_t m2_inference_back_dev(const m2_model* model, int32_t B, int32_t S, int32_t T_cap,
                              const int32_t* dev_T, const void* front, size_t front_bytes,
                              float* out_mel, float* out_audio, void* workspace,
                              size_t workspace_bytes, void* stream);
int32_t m2_frames_wait(const m2_model* model, void* stream, int32_t* host_T);

/* Ragged batches: every utterance as if synthesized alone.  frames [B] (int32,
 * device) holds utterance b's own frame count T_b; T (>= every T_b; values are
 * clamped to [1, T]) is the row stride of the [B,T,*] tensors.  Utterance b's
 * valid region - mel[b, :T_b] and audio[b, :64 T_b] - is what the B=1 call at
 * T_b frames computes (same kernels; the last 3 frames of a shorter
 * utterance's audio are computed again at its own length: by a second call of
 * the selected vocoder kernels on the batch's [B, 6]-frame end windows, or,
 * for an utterance of fewer than 6 frames, in fp32 by direct convolution,
 * within the parity tolerance of the MFMA kernels as the range policy's local
 * redo is); everything past it is exactly 0.  A batch whose T_b all equal T
 * gives the bits of the plain entry points.
 *   m2_mel_decoder_ragged: x [B,T,H] (rows past T_b are not read) -> mel.
 *   m2_vocoder_ragged: mel [B,M,T] / [B,T,M] (rows past T_b do not reach the
 *     valid audio, and are left as they are) -> audio [B,1,64T].  Any vocoder
 *     selection, also streamed (m2_vocoder_set_chunking).
 *   m2_inference_back_ragged: m2_inference_back at T = max(1, T_max) of
 *     m2_inference_front with T_b = max(1, total[b]) from the front buffer,
 *     also written to out_frames [B] (int32, device).
 * Workspaces: m2_mel_decoder_ragged as m2_mel_decoder; m2_vocoder_ragged
 * m2_workspace_bytes(B,0,T) + m2_ragged_workspace_bytes(B) and
 * m2_inference_back_ragged m2_inference_workspace_bytes(B,S,T) +
 * m2_ragged_workspace_bytes(B) (the end windows' vocoder pass).  M2_E_SHAPE
 * when the model's decoder does not run the one-launch layers (hidden_dim 32 /
 * 64 / 96 with 2 heads, M2_TF_LAYER=0) or its vocoder is not a fused one: the
 * caller then runs the utterances one by one. */
size_t m2_ragged_workspace_bytes(const m2_model* model, int32_t B);
int32_t m2_mel_decoder_ragged(const m2_model* model, const float* x, const int32_t* frames, int32_t B,
                              int32_t T, float* out_mel, void* workspace, size_t workspace_bytes,
                              void* stream);
int32_t m2_vocoder_ragged(const m2_model* model, const float* mel, int32_t mel_layout,
                          const int32_t* frames, int32_t B, int32_t T, float* out_audio,
                          void* workspace, size_t workspace_bytes, void* stream);
int32_t m2_inference_back_ragged(const m2_model* model, int32_t B, int32_t S, int32_t T,
                                 const void* front, size_t front_bytes, float* out_mel,
                                 float* out_audio, int32_t* out_frames, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* ---- kernel-level entry points (for the components API and tests) ---------*/

/* LightweightResBlock.forward (components.py:196-200) of vocoder stage k
 * (0..3): y = conv2(leaky(conv1(x))) + x.  x,y [B,c_k,L]; tmp: B*c_k*L floats. */
int32_t m2_vocoder_resblock(const m2_model* model, int32_t k, const float* x, int32_t B, int32_t L,
                            float* y, float* tmp, void* stream);

/* leaky(ConvTranspose1d) of vocoder stage k (tts_model.py:255-263, 291):
 * x [B,c,L] -> y [B,c/2,r*L]. */
int32_t m2_vocoder_upsample(const m2_model* model, int32_t k, const float* x, int32_t B, int32_t L,
                            float* y, void* stream);

/* Standalone kernels with caller-supplied weights in PyTorch layout (used by
 * the components API for modules that live outside an M2TTSModel). */

/* y = act((conv1d(x; w [Cout,Cin,ksize], b [Cout], padding ksize/2) [* alpha + beta]))
 * (+ res).  ksize 1 or 3; alpha/beta per output channel (the BatchNorm1d eval
 * form, components.py:170-171) or NULL; act 0 none, 1 leaky(0.1), 2 tanh,
 * 3 relu, 4 softplus(beta=1, threshold=20).  x [B,Cin,L], y/res [B,Cout,L].
 * Serves Conv1d in ConvBlock, VariancePredictor.projection, the vocoder's
 * input/output convs and LightweightResBlock convs used outside a model. */
int32_t m2_conv1d(const float* x, const float* w, const float* b, const float* alpha,
                  const float* beta, const float* res, int32_t ksize, int32_t act, int32_t B,
                  int32_t Cin, int32_t Cout, int32_t L, float* y, void* stream);

/* m2_conv1d for any kernel size, dilation and zero padding (components.py:
 * 143-200 ConvBlock(kernel_size), LightweightResBlock(kernel_size, dilation),
 * tts_model.py:246,272 SimpleVocoder(kernel_size)): y [B,Cout,Lo] with
 * Lo = L + 2*padding - dilation*(ksize-1); res (optional) needs Lo == L. */
int32_t m2_conv1d_ex(const float* x, const float* w, const float* b, const float* alpha, const float* beta,
                     const float* res, int32_t ksize, int32_t dilation, int32_t padding, int32_t act, int32_t B,
                     int32_t Cin, int32_t Cout, int32_t L, float* y, void* stream);

/* y = act(convT1d(x; w [Cin,Cout,2r], b, stride r, padding r/2)), r in {2,4};
 * x [B,Cin,L] -> y [B,Cout,r*L] (tts_model.py:255-263, 291). */
int32_t m2_conv_transpose1d(const float* x, const float* w, const float* b, int32_t rate,
                            int32_t act, int32_t B, int32_t Cin, int32_t Cout, int32_t L, float* y,
                            void* stream);

/* y[R,N] = act(LN?(x)[R,K] . w[N,K]^T + b) (+ res[R,N]).  gamma/beta NULL:
 * no LayerNorm (eps 1e-5); b may be NULL; act 0 none, 3 relu. */
int32_t m2_linear(const float* x, const float* gamma, const float* beta, const float* w,
                  const float* b, const float* res, int32_t act, int32_t R, int32_t K, int32_t N,
                  float* y, void* stream);

/* y[R,K] = LN(x) with affine gamma/beta, eps 1e-5. */
int32_t m2_layer_norm(const float* x, const float* gamma, const float* beta, int32_t R, int32_t K,
                      float* y, void* stream);

/* Attention core of MultiHeadAttention.forward (components.py:72-86):
 * qkv [B,N,3H] laid out (3, heads, hd) per row as the reference's reshape
 * implies; key_mask [B,N] uint8 or NULL (masked keys score -1e9);
 * out [B,N,H] (heads re-interleaved, before out_proj).  head_dim 16/32/48/64
 * run on the MFMA kernels, any other head_dim <= 256 on a generic fp32 one. */
int32_t m2_attention(const float* qkv, const uint8_t* key_mask, int32_t B, int32_t N, int32_t H,
                     int32_t heads, float* out, void* stream);

/* TextEncoder embedding (tts_model.py:78-80): y[b,s,:] = emb[ids[b,s],:] *
 * scale + pe[s,:] (scale = sqrt(H) as fp32); ids outside [0,vocab) read zeros. */
int32_t m2_embed_positional(const int64_t* ids, const float* emb, const float* pe, int32_t B,
                            int32_t S, int32_t H, int32_t vocab, float scale, float* y,
                            void* stream);

/* PositionalEncoding.forward (components.py:30-39): y = x + pe[:S] (x [B,S,H]). */
int32_t m2_add_positional(const float* x, const float* pe, int32_t B, int32_t S, int32_t H,
                          float* y, void* stream);

/* ---- mel features and Griffin-Lim (src/utils/audio.py:45-151) --
 * The reference's librosa calls: compute_mel_spectrogram = melspectrogram
 * (periodic Hann, centre zero padding, Slaney mel filters, power 2) ->
 * power_to_db(ref=max, amin 1e-10, top_db 80) -> [-1, 1] normalisation, per
 * utterance; mel_to_audio = (x+1)/2 -> db_to_power -> NNLS against the mel
 * filters (mel_to_stft; here Nesterov projected gradient from the clipped
 * pseudo-inverse - librosa uses scipy L-BFGS-B from the same start) -> sqrt
 * -> griffinlim(n_iter, momentum) -> istft -> / max|y|.
 *   m2_dsp_create: the tables (window, twiddles, mel filters, pseudo-inverse)
 *     for one (sr, n_fft in {512, 1024, 2048}, hop, win_length, n_mels, fmin,
 *     fmax); synchronises `stream`.
 *   audio [B, L] fp32; frames T = m2_dsp_frames(L) = 1 + L / hop;
 *   m2_stft -> complex64 [B, T, n_fft/2 + 1]; m2_mel_spectrogram -> out_mel
 *     [B, n_mels, T] normalised dB;
 *   m2_griffin_lim: from mel [B, n_mels, T] (normalised dB; magnitudes as
 *     m2_mel_to_magnitude) or, when mag != NULL, from magnitudes
 *     [B, T, n_fft/2+1] (bare griffinlim, no peak normalisation);
 *     init_angles complex64 [B, T, n_fft/2+1] unit phases (librosa's
 *     init='random' draw, made explicit); out_audio [B, hop (T - 1)]. */
typedef struct m2_dsp m2_dsp;
int32_t m2_dsp_create(int32_t sample_rate, int32_t n_fft, int32_t hop_length, int32_t win_length,
                      int32_t n_mels, float fmin, float fmax, void* stream, m2_dsp** out);
int32_t m2_dsp_destroy(m2_dsp* dsp);
int32_t m2_dsp_frames(const m2_dsp* dsp, int32_t L);
int32_t m2_stft(const m2_dsp* dsp, const float* audio, int32_t B, int32_t L, void* out_spec, void* stream);
int32_t m2_mel_spectrogram(const m2_dsp* dsp, const float* audio, int32_t B, int32_t L, float* out_mel,
                           void* stream);
/* compute_mel_spectrogram over a ragged batch: B utterances of unequal length
 * packed back to back, each featurized as if alone (the dB reference, the
 * top_db floor and the min/max are per utterance and taken over all of its
 * frames), written as the padded batch a collate function builds.
 *   samples: sample_format M2_SAMPLES_F32 (float32) or M2_SAMPLES_I16 (PCM16,
 *     read as (float)s / 32768.f); utterance b is samples[offsets[b],
 *     offsets[b + 1]), L_b of them, frames T_b = 1 + L_b / hop;
 *   offsets: int64 [B + 1] from 0, on the device, and the same values on the
 *     host in offsets_host: shapes and grids come from the host copy, so the
 *     call neither counts on the device nor synchronises;
 *   normalize != 0: x / max|x| per utterance in float32 when the peak is
 *     > 0, else unchanged (load_audio(normalize=True), audio.py:34-36);
 *   max_frames > 0: only each utterance's first max_frames frames are stored
 *     (the statistics still cover all T_b frames); 0 stores all;
 *   out_mel [B, n_mels, T_out]: utterance b's min(T_b, max_frames) frames,
 *     every column behind them exactly 0; out_frames int32 [B]: that count.
 * Utterance b equals, bit for bit, the leading columns of m2_mel_spectrogram
 * of its float32 signal alone, and two calls give equal bits (the only
 * atomic is an integer max).  M2_E_SHAPE: an L_b of 0, a T_out smaller than
 * the largest stored count, or total samples or n_mels x total frames
 * reaching 2^31 (split the corpus into several calls).
 * Scratch: m2_mel_features_ragged_workspace_bytes(B, total samples).  Like
 * every *_workspace_bytes of the DSP, evaluation and loss calls below, the
 * returned size is exact up to 256 bytes of slack. */
#define M2_SAMPLES_F32 0
#define M2_SAMPLES_I16 1
size_t m2_mel_features_ragged_workspace_bytes(const m2_dsp* dsp, int32_t B, int64_t total_samples);
int32_t m2_mel_features_ragged(const m2_dsp* dsp, const void* samples, int32_t sample_format,
                               const int64_t* offsets, const int64_t* offsets_host, int32_t B,
                               int32_t normalize, int32_t max_frames, float* out_mel, int32_t T_out,
                               int32_t* out_frames, void* workspace, size_t workspace_bytes, void* stream);
/* mel_to_stft alone (librosa.feature.inverse.mel_to_stft, power 2, as
 * audio.py:138 reaches it): mel [B, n_mels, T] -> magnitudes out_mag
 * [B, T, n_fft/2+1] = sqrt(librosa.util.nnls(mel_basis, db_to_power)).
 * librosa's L-BFGS-B stops at its start X0 = max(0, pinv(W) M) whenever the
 * block's projected gradient there is <= 1e-5 (every mel in the normalised
 * range); that test is made exactly and X0 returned; a block that would
 * iterate gets nnls_iters projected-gradient steps per frame instead.
 * Scratch: m2_mel_to_magnitude_workspace_bytes. */
size_t m2_mel_to_magnitude_workspace_bytes(const m2_dsp* dsp, int32_t B, int32_t T);
int32_t m2_mel_to_magnitude(const m2_dsp* dsp, const float* mel, int32_t B, int32_t T, int32_t nnls_iters,
                            float* out_mag, void* workspace, size_t workspace_bytes, void* stream);
size_t m2_griffin_lim_workspace_bytes(const m2_dsp* dsp, int32_t B, int32_t T);
int32_t m2_griffin_lim(const m2_dsp* dsp, const float* mel, const float* mag, const void* init_angles,
                       int32_t B, int32_t T, int32_t n_iter, float momentum, int32_t nnls_iters,
                       float* out_audio, void* workspace, size_t workspace_bytes, void* stream);

/* ---- evaluation metrics (src/evaluation/metrics.py) -------------------------
 * Per-utterance rows of double sums; the scalar finishing of the reference's
 * metrics (log10, clips, MOS weights, correlation) is the caller's.  Columns
 * are named: m2_eval_column_count(kind) / m2_eval_column_name(kind, i), kind
 * 0 = m2_eval_audio, 1 = m2_eval_pair_stats, 2 = m2_eval_mcd.  All reductions
 * run in a fixed order, so equal inputs give equal bits.
 *
 * m2_eval_audio: estimate_mos_score's sums (metrics.py:79-148, with
 * compute_spectral_convergence and compute_log_spectral_distance, :27-58) for
 * pred [B, Lp] and target [B, Lt] (NULL: reference-free), STFT n_fft / hop /
 * window / sample rate of `dsp`.  With L = min(Lp, Lt) and X(.) the STFT of
 * the first L samples (1 + L / hop frames):
 *   spec_err_sq  sum (|X(target)| - |X(pred)|)^2     spec_ref_sq  sum |X(target)|^2
 *   log_spec_sq  sum (ln(|X(pred)| + 1e-8) - ln(|X(target)| + 1e-8))^2
 *   pair_bins    their count, (1 + L / hop) (n_fft / 2 + 1)
 *   target_sq, noise_sq   sum target^2, sum (pred - target)^2 over [0, L); pair_len = L
 *   pred_sq, sign_changes sum pred^2 and sum |sign(x[i+1]) - sign(x[i])| over
 *                the whole pred (sign(0) = 0); pred_len = Lp
 *   centroid_sum, bandwidth_sum  sums over the whole pred's pred_frames =
 *                1 + Lp / hop frames of librosa's spectral_centroid and
 *                spectral_bandwidth (p = 2) of the magnitude spectrum
 * The columns that need a target are 0 without one.  B <= 65535.
 *
 * m2_eval_pair_stats: target [B, R, C]; pred [B, R, C], or [B, C, R] read
 * transposed (the model's mel [B, T, M] against a target [B, M, T]); cols
 * (int32 [B] or NULL) keeps each utterance's first min(cols[b], C) columns
 * (metrics.py:244-248).  Per utterance abs_diff = sum |p - t|, sq_diff,
 * sum_p, sum_t, sum_pp, sum_tt, sum_pt, count, and the centred second moments
 * cen_pp = sum (p - mean p)^2, cen_tt, cen_pt (a constant row gives exactly 0).
 * compute_mel_distance (:15-24) and compute_duration_accuracy (:151-177, R = 1).
 *
 * m2_eval_mcd: compute_mcd (:61-76): target [B, M, Tt]; pred [B, M, Tp] or
 * [B, Tp, M]; over the first min(Tp, Tt, cols[b]) frames, mcd_sum = sum of
 * sqrt(sum_c (D (pred - target))_c^2) with D = `table`, device doubles
 * [m2_eval_mcd_coefficients() = 13, M]: the first rows of the orthonormal
 * DCT-II (librosa.feature.mfcc(S=., n_mfcc=13) takes no dB step), which
 * m2_eval_dct_table writes to HOST memory for the caller to upload. */
int32_t m2_eval_column_count(int32_t kind);
const char* m2_eval_column_name(int32_t kind, int32_t index);
size_t m2_eval_audio_workspace_bytes(const m2_dsp* dsp, int32_t B, int32_t Lp);
int32_t m2_eval_audio(const m2_dsp* dsp, const float* pred, const float* target, int32_t B, int32_t Lp,
                      int32_t Lt, double* out, void* workspace, size_t workspace_bytes, void* stream);
int32_t m2_eval_pair_stats(const float* pred, const float* target, const int32_t* cols, int32_t B, int32_t R,
                           int32_t C, int32_t pred_transposed, double* out, void* stream);
int32_t m2_eval_mcd_coefficients(void);
int32_t m2_eval_dct_table(int32_t n_mels, double* out_host);
int32_t m2_eval_mcd(const float* pred, const float* target, const int32_t* cols, const double* table, int32_t B,
                    int32_t n_mels, int32_t Tp, int32_t Tt, int32_t pred_transposed, double* out, void* stream);

/* ---- training losses (src/training/losses.py) ------------------------------
 * Forward values, the backward of the discriminator step (the gradient of
 * the adversarial discriminator loss with respect to the discriminators'
 * parameters), and the generator step's gradients with respect to the audio:
 * through the discriminators, and of the spectral and perceptual sums.
 * Per-utterance rows of double sums as above, columns named by
 * m2_loss_column_count(kind) / m2_loss_column_name(kind, i): kind 0 =
 * m2_loss_spectral, 1 = m2_disc_losses.  Fixed-order reductions: equal inputs
 * give equal bits, and a batched row equals the row of the utterance alone.
 *
 * m2_conv1d_strided: y = leaky(conv1d(x; w [Cout, Cin/groups, k], b (or NULL),
 * stride, zero padding, groups), slope), leaky(v) = v > 0 ? v : slope v
 * (slope 1: no activation; the discriminators use 0.2).  x [B,Cin,L] ->
 * y [B,Cout,(L + 2 padding - k)/stride + 1]; groups divides both channel
 * counts.  Cout >= 16 with (Cin/groups) k >= 32 runs on the exact-f32 MFMA.
 * m2_avg_pool1d: F.avg_pool1d(x [B,C,L], k, stride k) -> [B,C,L/k] (the tail
 * samples are dropped).
 *
 * m2_disc: the discriminators of one MultiScaleDiscriminator (losses.py:59-117,
 * seven Conv1d each), packed once from `weights`: n_scales * 14 device
 * pointers in state_dict order (weight, bias per layer; PyTorch layouts).
 * Scale s reads avg_pool1d(x, scales[s]).
 *   m2_disc_layer_shape: channels and length of layer `layer` (0..6) of scale
 *     index s for audio of L samples.
 *   m2_disc_layer: one packed layer on its own: x [B,Cin,L] (the previous
 *     layer's output, or the pooled audio for layer 0) -> y [B,Cout,len],
 *     LeakyReLU(0.2) applied to x for layer > 0, none to y.
 *   m2_disc_forward: x [B,1,L] -> logits: the last layers' outputs
 *     [B,1,len(s,6)], scale after scale; features (or NULL): the six other
 *     layers' outputs [B,C,len(s,l)] before the LeakyReLU(0.2), as the
 *     reference collects them (losses.py:109-112; the next layer's loader
 *     applies the slope), scale-major, layer-minor, each contiguous.
 *   m2_disc_losses: real and/or fake [B,1,L] (NULL: absent, its sums are 0) ->
 *     out [B, K].  Per scale: s<i>_real_err_sq = sum (D(real) - 1)^2,
 *     s<i>_real_sq, s<i>_fake_err_sq, s<i>_fake_sq, s<i>_logits (their count);
 *     per scale and layer: s<i>_l<j>_abs_diff = sum |f_fake - f_real|,
 *     s<i>_l<j>_count.  Three scales.  No feature map leaves the workspace.
 *   Both walk the batch in slices whose activations fit m2_disc_set_slice_bytes
 *   (default, and 0: 1 GiB - B = 32 utterances of 32000 samples in one slice;
 *   at least one utterance per slice); the workspace queries follow it.
 *
 * m2_loss_spectral: pred, target [B,L] through torch.stft(n_fft, hop,
 * center=True, pad_mode='reflect', periodic Hann) of the handle's n_fft and
 * hop (L > n_fft/2).  Per utterance mag_abs = sum | |P| - |T| |, phase_abs =
 * sum |angle P - angle T|, bins, mel_log_abs = sum over frames and the
 * n_weights weights w_j (device floats, or NULL with 0) of |ln(w_j sum_f |P| +
 * 1e-8) - ln(w_j sum_f |T| + 1e-8)| (PerceptualLoss._mel_features: its filter
 * rows are constant), frames.  spec_pred / spec_target (or NULL): the
 * complex64 spectra [B, frames, n_fft/2+1] the sums were taken from; DC and
 * Nyquist bins have imaginary part +0.
 *
 * m2_conv1d_strided_backward: the gradients of one layer
 * y = conv1d(leaky(x_pre, in_slope); w, b; k, stride, padding, groups) given
 * dy [B,Cout,Lo], the cotangent of y: dx (or NULL) [B,Cin,L], the cotangent of
 * x_pre (leaky'(v) = v > 0 ? 1 : in_slope, the forward's predicate; exactly 0
 * at positions no output read); dw [Cout, Cin/groups, k] and db (or NULL)
 * [Cout], summed over the batch.  Outputs are overwritten.  w and dw are in
 * PyTorch's layout.  Same generality as m2_conv1d_strided (Cin at most
 * 65535); the geometries m2_conv1d_strided runs on the MFMA get dx from it
 * (Cin >= 16), every Cout >= 16 gets dw from it, split over K into partials
 * in the workspace that are added in a fixed order (no floating-point
 * atomics: equal inputs give equal bits); the rest run one thread per dx
 * sample and one workgroup per dw element.
 *
 * m2_disc_step: m2_disc_losses's `out` (same launches, same bits; real and
 * fake are both required) and, in grads (n_scales * 14 device pointers in
 * state_dict order, PyTorch layouts, overwritten), the gradient of
 *   L_D = (1/n_scales) sum_s [ mean (D_s(real) - 1)^2 + mean D_s(fake)^2 ]
 * with respect to every weight and bias.  The logit cotangents
 * 2 (D - 1) / (N_s n_scales) and 2 D / (N_s n_scales), N_s = B len(s,6), need
 * no pass of their own: each (slice, scale) runs forward, then each side
 * backward while its maps are in the workspace, and the gradients accumulate
 * over slices and sides in stream order.  m2_disc_set_slice_bytes gives the
 * slices of m2_disc_losses (the bound counts the maps of both sides); the
 * workspace query adds two cotangent maps of the widest layer and the pooled
 * audio per utterance of a slice, and the split-K partials (at most 32 MiB
 * beyond one copy of the largest weight).
 *
 * m2_disc_gen_step: the generator step's gradient through the
 * discriminators.  `out` as m2_disc_losses writes it (same launches, same
 * bits) and d_fake [B,1,L] (overwritten), the gradient with respect to `fake`
 * of
 *   w_adv L_G + w_fm L_FM,
 *   L_G  = (1/3) sum_s mean (D_s(fake) - 1)^2,
 *   L_FM = (1/18) sum_{s,j} mean |f_{s,j}(fake) - f_{s,j}(real)|,
 * f_{s,j} the six pre-activation maps of scale s.  real may be NULL exactly
 * when w_fm == 0: only the fake side runs then, and `out` is
 * m2_disc_losses(NULL, fake)'s (NULL with w_fm != 0 is M2_E_ARG).  Each
 * (slice, scale) runs forward, then the fake side backward while the maps of
 * both sides are in the workspace: the logit cotangent
 * w_adv 2 (D - 1) / (3 N_s), the data gradients of layers 6..1 (no weight,
 * bias or split-K launch), w_fm sign(f_fake - f_real) / (18 count(s,j)) added
 * to the cotangent of map j before the layer below reads it (sign(0) = 0, as
 * torch's l1_loss backward), and the first layer fused with the adjoint of
 * avg_pool1d: d_pooled[u] / scale on samples u scale .. u scale + scale - 1,
 * nothing on the samples floor pooling dropped.  Scale index 0 overwrites a
 * slice's rows of d_fake, the later scales add in stream order; no kernel
 * reduces over the batch, so the slice size does not change a bit.  real and
 * the discriminators' parameters get no gradient.  Slices as m2_disc_losses;
 * the workspace query adds the two cotangent maps of m2_disc_step.
 *
 * m2_conv1d_audio_backward: that last kernel on its own: the gradient of
 * y = conv1d(avg_pool1d(x, pool); w [Cout,1,k], stride 1, padding) with
 * respect to x [B,1,L], given dy [B,Cout,L/pool + 2 padding - k + 1]; dx
 * [B,1,L] is overwritten (the dropped tail samples with 0) or, with
 * `accumulate`, added to (the tail left alone).  Cout k floats of weights and
 * a 16-channel window of 256 + k - 1 samples must fit 48 KiB of LDS.
 *
 * m2_loss_spectral_backward: d_pred [B,L], the gradient with respect to pred of
 *   c_mag mag_abs + c_phase phase_abs + c_perc mel_log_abs
 * summed over the batch (m2_loss_spectral's columns at the handle's n_fft and
 * hop; host coefficients, so a mean is 1 / count), overwritten or, with
 * `accumulate`, added to as one fp32 addition per sample.  Same arguments,
 * limits and framing as m2_loss_spectral, and the same spectra bit for bit.
 * Per bin the cotangent g = d/dRe P + i d/dIm P is formed in double and rounded
 * once: (c_mag sign(|P| - |T|) + kappa_t) P/|P| + c_phase sign(angle P -
 * angle T) (-Im P + i Re P)/|P|^2, kappa_t = c_perc sum_j sign(ln(w_j S_P +
 * 1e-8) - ln(w_j S_T + 1e-8)) w_j / (w_j S_P + 1e-8), S_X = sum_f |X_f|;
 * sign(0) = 0, and g = 0 where |P| = 0 (torch's abs and angle backward).  The
 * derivative is taken on the kernel's own fp32 spectrum.  A frame's cotangent
 * is win[n] Re sum_{f <= n_fft/2} g_f e^(+2 pi i f n / n_fft), held in the
 * workspace ([B, frames, n_fft] floats); each sample then gathers padded
 * positions i, -i and 2 (L - 1) - i (the adjoint of reflect padding), frames
 * ascending, in fp32.  No floating-point atomics: equal inputs give equal bits
 * and a batched row equals the row of the utterance alone.  cot_pred (or
 * NULL): g as complex64 [B, frames, n_fft/2+1].  target gets no gradient. */
typedef struct m2_disc m2_disc;
int32_t m2_loss_column_count(int32_t kind);
const char* m2_loss_column_name(int32_t kind, int32_t index);
int32_t m2_conv1d_strided(const float* x, const float* w, const float* b, int32_t ksize, int32_t stride,
                          int32_t padding, int32_t groups, float leaky_slope, int32_t B, int32_t Cin, int32_t Cout,
                          int32_t L, float* y, void* stream);
int32_t m2_avg_pool1d(const float* x, int32_t ksize, int32_t B, int32_t C, int32_t L, float* y, void* stream);
int32_t m2_disc_create(const float* const* weights, int32_t count, const int32_t* scales, int32_t n_scales,
                       void* stream, m2_disc** out);
int32_t m2_disc_destroy(m2_disc* disc);
int32_t m2_disc_set_slice_bytes(m2_disc* disc, size_t bytes);
int32_t m2_disc_layer_shape(const m2_disc* disc, int32_t L, int32_t scale_index, int32_t layer, int32_t* channels,
                            int32_t* length);
int32_t m2_disc_layer(const m2_disc* disc, int32_t scale_index, int32_t layer, const float* x, int32_t B, int32_t L,
                      float* y, void* stream);
/* The *_workspace_bytes below: the returned size is exact up to 256 bytes of slack. */
size_t m2_disc_forward_workspace_bytes(const m2_disc* disc, int32_t B, int32_t L);
int32_t m2_disc_forward(const m2_disc* disc, const float* x, int32_t B, int32_t L, float* logits, float* features,
                        void* workspace, size_t workspace_bytes, void* stream);
size_t m2_disc_losses_workspace_bytes(const m2_disc* disc, int32_t B, int32_t L);
int32_t m2_disc_losses(const m2_disc* disc, const float* real, const float* fake, int32_t B, int32_t L, double* out,
                       void* workspace, size_t workspace_bytes, void* stream);
size_t m2_conv1d_strided_backward_workspace_bytes(int32_t ksize, int32_t stride, int32_t padding, int32_t groups,
                                                  int32_t B, int32_t Cin, int32_t Cout, int32_t L);
int32_t m2_conv1d_strided_backward(const float* x_pre, const float* w, const float* dy, int32_t ksize, int32_t stride,
                                   int32_t padding, int32_t groups, float in_slope, int32_t B, int32_t Cin,
                                   int32_t Cout, int32_t L, float* dx, float* dw, float* db, void* workspace,
                                   size_t workspace_bytes, void* stream);
size_t m2_disc_step_workspace_bytes(const m2_disc* disc, int32_t B, int32_t L);
int32_t m2_disc_step(const m2_disc* disc, const float* real, const float* fake, int32_t B, int32_t L, double* out,
                     float* const* grads, void* workspace, size_t workspace_bytes, void* stream);
size_t m2_disc_gen_step_workspace_bytes(const m2_disc* disc, int32_t B, int32_t L);
int32_t m2_disc_gen_step(const m2_disc* disc, const float* real, const float* fake, int32_t B, int32_t L,
                         double w_adv, double w_fm, double* out, float* d_fake, void* workspace,
                         size_t workspace_bytes, void* stream);
int32_t m2_conv1d_audio_backward(const float* dy, const float* w, int32_t ksize, int32_t padding, int32_t pool,
                                 int32_t B, int32_t Cout, int32_t L, int32_t accumulate, float* dx, void* stream);
size_t m2_loss_spectral_workspace_bytes(const m2_dsp* dsp, int32_t B, int32_t L);
int32_t m2_loss_spectral(const m2_dsp* dsp, const float* pred, const float* target, int32_t B, int32_t L,
                         const float* mel_weights, int32_t n_weights, double* out, void* spec_pred, void* spec_target,
                         void* workspace, size_t workspace_bytes, void* stream);
size_t m2_loss_spectral_backward_workspace_bytes(const m2_dsp* dsp, int32_t B, int32_t L);
int32_t m2_loss_spectral_backward(const m2_dsp* dsp, const float* pred, const float* target, int32_t B, int32_t L,
                                  const float* mel_weights, int32_t n_weights, double c_mag, double c_phase,
                                  double c_perc, int32_t accumulate, float* d_pred, void* cot_pred, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* ---- vocoder training: a forward that keeps a tape, and the backward ---------
 * The gradient of SimpleVocoder (kernel size 3) with respect to its 28
 * parameters and its input mel, exact f32, without a model handle: an
 * optimizer step changes every parameter, so these calls read the parameters
 * where they are.  params: 28 device pointers in state_dict order and PyTorch
 * layouts (input_conv.{weight,bias}, upsamples.k.{weight,bias},
 * resblocks.k.conv1.{weight,bias}, resblocks.k.conv2.{weight,bias},
 * output_conv.{weight,bias}; ConvTranspose1d weights [Cin, Cout, 2r]).
 * Shapes: mel [B,M,T], M >= 1; C a multiple of 16 in [16, 256]; at most 65535
 * utterances, 2^22 frames each and 2^24 in all (else M2_E_SHAPE).  B = 0 or
 * T = 0 launches nothing and returns M2_OK.  No call synchronises.
 *
 * m2_vocoder_train_forward: audio [B,1,64T], bit for bit what a stand-alone
 * SimpleVocoder's per-op forward gives (the same kernels, m2_conv1d and
 * m2_conv_transpose1d with their fused activation and residual), each layer
 * writing into the tape.  The tape holds 14 float32 maps [B, channels,
 * length], each on a 256-byte boundary (m2_vocoder_tape_map: offset in floats
 * from the tape's base), c_k = C / 2^(k+1), L_k = T x 4, 16, 32, 64:
 *   0       h      [C, T]      input_conv(mel)
 *   1 + 3k  a_k    [c_k, L_k]  leaky(ConvT_k(x_k), 0.1), post-activation
 *   2 + 3k  lv_k   [c_k, L_k]  leaky(conv1_k(a_k), 0.1), post-activation
 *   3 + 3k  x_k+1  [c_k, L_k]  conv2_k(lv_k) + a_k
 *   13      y      [1, 64 T]   the audio (tanh' = 1 - y^2)
 * Slope 0.1 keeps the sign, so the backward reads LeakyReLU's predicate
 * (value > 0) from the stored value.  About 10.7 MB per utterance at stage1,
 * T = 500.  A tape smaller than m2_vocoder_tape_bytes is M2_E_ARG.
 *
 * m2_vocoder_backward: given d_audio [B,1,64T], the cotangent of the audio,
 * d_mel [B,M,T] (or NULL: the input conv's data gradient is skipped;
 * otherwise always overwritten) and grads: 28 device pointers shaped like the
 * parameters, each overwritten or, with `accumulate`, added to as one fp32
 * addition per element; a NULL entry skips that tensor.  mel, params and the
 * tape are those of the forward call.  No floating-point atomics: weight and
 * bias gradients reduce over (utterance, position) through partials in the
 * workspace that are added in a fixed order, so equal inputs give equal bits;
 * d_mel has no reduction over the batch, so a batched row equals the row of
 * the utterance computed alone.  A workspace smaller than
 * m2_vocoder_backward_workspace_bytes is M2_E_ARG (two cotangent maps and g_v
 * of the widest layer, 4 C T floats per utterance each, the partials, and one
 * weight and one bias of the largest size: with `accumulate` a gradient is
 * formed there exactly as without it and then added onto the caller's).
 * The launches: voc_out_bwd_kernel (tanh', the output conv's data gradient and
 * its weight / bias partials in one pass), per stage voc_res_dx_kernel (the
 * resblock's data gradient, conv2^T(g_r) and g_a kept in LDS), the weight
 * gradients on the exact-f32 MFMA (m2_conv1d_strided_backward's kernels) or,
 * below 16 output channels, voc_dw_narrow_kernel, and the ConvTranspose1d's
 * gradients as those of the strided Conv1d with the roles swapped
 * (m2_conv1d_strided on g_u with the ConvT weight read as [Cout', Cin', 2r]).
 *
 * m2_debug_vocoder_grad_plan: the tape and workspace sizes and every launch
 * of m2_vocoder_backward(M, C, B, T) with all gradients asked for, as one
 * line of text (the format is fixed and documented in
 * csrc/vocoder_grad_plan.h).  Host arithmetic only.  Writes at most cap bytes
 * (NUL-terminated) and returns the line's length, or a negative M2_E_* code.
 *
 * The three kernels alone:
 * m2_vocoder_out_backward: y = tanh(conv(x [B,c,L]; w [1,c,3], padding 1) + b),
 *   gy and y [B,1,L] -> gx [B,c,L], dw [1,c,3], db [1] (each may be NULL),
 *   overwritten.
 * m2_resblock_backward: x_out = conv2(lv) + a, lv = leaky(conv1(a)), all
 *   [B,c,L], c <= 128, w1 and w2 [c,c,3]; from g_r, the cotangent of x_out,
 *   g_v (the cotangent of conv1's output) and g_u = leaky'(a) x the cotangent
 *   of a.
 * m2_conv1d_narrow_dw: dw [Cout,Cin,k] and db [Cout] (either may be NULL) of
 *   y = conv1d(x [B,Cin,L]; stride, padding) + b given dy, overwritten, for
 *   Cout < 16 and
 *   windows that fit 48 KiB of LDS (else M2_E_SHAPE; the query returns 0). */
size_t m2_vocoder_tape_bytes(int32_t M, int32_t C, int32_t B, int32_t T);
int32_t m2_vocoder_tape_map(int32_t M, int32_t C, int32_t B, int32_t T, int32_t index, size_t* offset_floats,
                            int32_t* channels, int32_t* length);
int32_t m2_vocoder_train_forward(const float* const* params, int32_t M, int32_t C, const float* mel, int32_t B,
                                 int32_t T, float* audio, void* tape, size_t tape_bytes, void* stream);
size_t m2_vocoder_backward_workspace_bytes(int32_t M, int32_t C, int32_t B, int32_t T);
int32_t m2_vocoder_backward(const float* const* params, int32_t M, int32_t C, const float* mel, int32_t B, int32_t T,
                            const void* tape, const float* d_audio, float* d_mel, float* const* grads,
                            int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);
int32_t m2_debug_vocoder_grad_plan(int32_t M, int32_t C, int32_t B, int32_t T, char* out, size_t cap);
size_t m2_vocoder_out_backward_workspace_bytes(int32_t B, int32_t c, int32_t L);
int32_t m2_vocoder_out_backward(const float* gy, const float* y, const float* x, const float* w, int32_t B, int32_t c,
                                int32_t L, float* gx, float* dw, float* db, void* workspace, size_t workspace_bytes,
                                void* stream);
int32_t m2_resblock_backward(const float* g_r, const float* lv, const float* a, const float* w1, const float* w2,
                             int32_t B, int32_t c, int32_t L, float* g_v, float* g_u, void* stream);
size_t m2_conv1d_narrow_dw_workspace_bytes(int32_t ksize, int32_t stride, int32_t padding, int32_t B, int32_t Cin,
                                           int32_t Cout, int32_t L);
int32_t m2_conv1d_narrow_dw(const float* x, const float* dy, int32_t ksize, int32_t stride, int32_t padding, int32_t B,
                            int32_t Cin, int32_t Cout, int32_t L, float* dw, float* db, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ---- the mel decoder's training forward and backward ----------------------
 * MelDecoder from its raw parameters (no model handle: an optimizer step
 * changes every one of them).  params: 11 layers + 4 device pointers in
 * state_dict order, PyTorch layout, read where they are: per layer
 * self_attn.qkv.weight [3H,H], self_attn.out_proj.weight [H,H] and .bias,
 * ffn.linear1.weight [2H,H] and .bias, ffn.linear2.weight [H,2H] and .bias,
 * norm1.weight, norm1.bias, norm2.weight, norm2.bias; then norm.weight,
 * norm.bias, mel_projection.weight [M,H] and .bias.  The dimension arguments
 * are (H, M, layers, heads, B, T); x is [B,T,H], read as R = B T rows.
 * Supported: H a multiple of 8 with 2 H <= 256, head_dim H / heads in
 * {16, 32, 48, 64}, M >= 1, layers >= 1 (else M2_E_SHAPE; the _bytes queries
 * return 0).  B = 0 or T = 0: nothing to do, M2_OK.
 *
 * m2_decoder_train_forward: mel [B,T,M], bit-equal to the stand-alone
 * module's forward (m2_linear with its fused LayerNorm / ReLU / residual and
 * m2_attention under the process's switches, in that order), each op writing
 * into the tape: per layer qkv [R,3H], att [R,H], x_mid [R,H], h [R,2H] (stored
 * post-ReLU) and x_out [R,H], each map on a 256-byte boundary.
 * m2_decoder_tape_map(index = 5 layer + map) names a map's offset (in floats)
 * and width.  A tape shorter than m2_decoder_tape_bytes: M2_E_ARG.
 *
 * m2_decoder_backward: given d_mel [B,T,M], d_x [B,T,H] (NULL: skipped) and
 * grads, 11 layers + 4 device pointers shaped like the parameters (a NULL entry
 * skips that tensor and its launches).  Each is overwritten, or with
 * accumulate != 0 added to: the gradient's partials are summed exactly as
 * without it and that sum is added with one fp32 addition per element.  Exact
 * f32 on v_mfma_f32_16x16x4_f32, no floating-point atomics: equal inputs give
 * equal bits, and a row of d_x depends on its own utterance only.  LayerNorm
 * statistics and attention probabilities are recomputed, not taped.  A
 * workspace shorter than m2_decoder_backward_workspace_bytes: M2_E_ARG.
 *
 * m2_debug_decoder_grad_plan: the tape and workspace sizes and every launch of
 * m2_decoder_backward with all gradients asked for, as one line of text (the
 * format is fixed and documented in csrc/decoder_grad_plan.h).  Host
 * arithmetic only.  Writes at most cap bytes (NUL-terminated) and returns the
 * line's length, or a negative M2_E_* code.
 *
 * The kernels alone:
 * m2_attention_backward: d_qkv [B,N,3H] (overwritten) of att = softmax(Q K^T /
 *   sqrt(hd), key_mask) V given qkv, att and d_att [B,N,H]; key_mask [B,N]
 *   (0 = masked; NULL: none).  A masked key's score is replaced, so its dS is 0
 *   by definition: in a fully masked row dQ and dK are exactly 0 and dV still
 *   receives P^T dO with P = 1 / N.  The workspace holds the row statistics.
 * m2_linear_backward_input: g_x [R,K] = g_y [R,N] w [N,K], K a multiple of 8,
 *   at most 256.  relu_of [R,K] (or NULL): g_x is multiplied by relu_of > 0.
 *   ln_x [R,K] with gamma [K] (or both NULL; K <= 128; not with relu_of): the
 *   product is the cotangent of LayerNorm(ln_x) and g_x is the LayerNorm's
 *   input cotangent plus g_res [R,K] (or NULL); dgamma and dbeta [K] (each may
 *   be NULL) are overwritten, through the workspace
 *   (m2_linear_backward_input_workspace_bytes); g_x may then be NULL.
 * m2_linear_backward_weight: dw [N,K] = g_y^T X and db [N] = sum_r g_y (either
 *   may be NULL), overwritten; X = x [R,K], or LayerNorm(x; ln_gamma, ln_beta)
 *   re-formed while loading when those are given. */
size_t m2_decoder_tape_bytes(int32_t H, int32_t M, int32_t layers, int32_t heads, int32_t B, int32_t T);
int32_t m2_decoder_tape_map(int32_t H, int32_t M, int32_t layers, int32_t heads, int32_t B, int32_t T, int32_t index,
                            size_t* offset_floats, int32_t* width);
int32_t m2_decoder_train_forward(const float* const* params, int32_t H, int32_t M, int32_t layers, int32_t heads,
                                 const float* x, int32_t B, int32_t T, float* mel, void* tape, size_t tape_bytes,
                                 void* stream);
size_t m2_decoder_backward_workspace_bytes(int32_t H, int32_t M, int32_t layers, int32_t heads, int32_t B, int32_t T);
int32_t m2_decoder_backward(const float* const* params, int32_t H, int32_t M, int32_t layers, int32_t heads,
                            const float* x, int32_t B, int32_t T, const void* tape, const float* d_mel, float* d_x,
                            float* const* grads, int32_t accumulate, void* workspace, size_t workspace_bytes,
                            void* stream);
int32_t m2_debug_decoder_grad_plan(int32_t H, int32_t M, int32_t layers, int32_t heads, int32_t B, int32_t T, char* out,
                                   size_t cap);
size_t m2_attention_backward_workspace_bytes(int32_t B, int32_t N, int32_t heads);
int32_t m2_attention_backward(const float* qkv, const uint8_t* key_mask, const float* att, const float* d_att,
                              int32_t B, int32_t N, int32_t H, int32_t heads, float* d_qkv, void* workspace,
                              size_t workspace_bytes, void* stream);
size_t m2_linear_backward_input_workspace_bytes(int32_t R, int32_t K);
int32_t m2_linear_backward_input(const float* g_y, const float* w, const float* relu_of, const float* ln_x,
                                 const float* gamma, const float* g_res, int32_t R, int32_t K, int32_t N, float* g_x,
                                 float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
size_t m2_linear_backward_weight_workspace_bytes(int32_t R, int32_t K, int32_t N);
int32_t m2_linear_backward_weight(const float* g_y, const float* x, const float* ln_gamma, const float* ln_beta,
                                  int32_t R, int32_t K, int32_t N, float* dw, float* db, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* ---- the text encoder's training forward and backward, the length regulator's
 * adjoint ------------------------------------------------------------------
 * TextEncoder from its raw parameters, as the decoder above.  params: 1 + 11
 * layers + 2 device pointers in parameters() order: embedding.weight [V,H],
 * the layers' 11 each (the decoder's), norm.weight, norm.bias.  The dimension
 * arguments are (V, H, layers, heads, B, S); ids is int64 [B,S], read as R = B S
 * positions; pe is the positional table's first S rows [S,H] (a buffer: it gets
 * no gradient); key_mask is [B,S] bytes (0 = masked) or NULL.  Supported: the
 * decoder's shapes and 1 <= V <= 65536 (else M2_E_SHAPE; the _bytes queries
 * return 0).  B = 0 or S = 0: nothing to do, M2_OK.
 *
 * m2_encoder_train_forward: out [B,S,H], bit-equal to the stand-alone module's
 * forward (m2_embed_positional at scale sqrt(H), the layers with the key mask,
 * m2_layer_norm), each op writing into the tape: x0 [R,H], the embedding's
 * output, then the decoder's five maps per layer.  m2_encoder_tape_map(index =
 * 0, or 1 + 5 layer + map) names a map's offset (in floats) and width.
 *
 * m2_encoder_backward: given d_out [B,S,H], grads as the decoder's (1 + 11
 * layers + 2 pointers, NULL skips, accumulate adds with one fp32 addition per
 * element).  An id outside [0, V) read a zero row and contributes nothing; a
 * vocabulary row that never occurs gets exactly 0.  No floating-point atomics:
 * equal inputs give equal bits.
 *
 * m2_debug_encoder_grad_plan: as m2_debug_decoder_grad_plan (the format is in
 * csrc/encoder_grad_plan.h).
 *
 * The kernels alone:
 * m2_embedding_backward: d_emb [V,H] = scale * the sum of d_x [R,H] over the
 *   positions with ids[r] == v, in ascending position; overwritten, or added
 *   to with accumulate != 0.  1 <= V <= 65536, H <= 256.
 * m2_layer_norm_backward: the backward of y = LayerNorm(x; gamma, beta), x and
 *   g_y [R,K], K a multiple of 8, at most 128: g_x [R,K] (or NULL) = the
 *   input's cotangent plus g_res [R,K] (or NULL); dgamma and dbeta [K] (each
 *   may be NULL) are overwritten, through the workspace.
 * m2_length_regulator_backward: the adjoint of m2_length_regulator_expand:
 *   d_enc [B,S,H] at (b, s) = the sum of d_reg [B,T_out,H] at (b, t) over
 *   cum[b,s] <= t < min(cum[b,s+1], T_out), t ascending, so the order depends on
 *   the phoneme's frame count alone; a phoneme without frames gets exactly 0,
 *   padding and truncated frames reach nothing, durations get no gradient. */
size_t m2_encoder_tape_bytes(int32_t V, int32_t H, int32_t layers, int32_t heads, int32_t B, int32_t S);
int32_t m2_encoder_tape_map(int32_t V, int32_t H, int32_t layers, int32_t heads, int32_t B, int32_t S, int32_t index,
                            size_t* offset_floats, int32_t* width);
int32_t m2_encoder_train_forward(const float* const* params, int32_t V, int32_t H, int32_t layers, int32_t heads,
                                 const int64_t* ids, const float* pe, const uint8_t* key_mask, int32_t B, int32_t S,
                                 float* out, void* tape, size_t tape_bytes, void* stream);
size_t m2_encoder_backward_workspace_bytes(int32_t V, int32_t H, int32_t layers, int32_t heads, int32_t B, int32_t S);
int32_t m2_encoder_backward(const float* const* params, int32_t V, int32_t H, int32_t layers, int32_t heads,
                            const int64_t* ids, const uint8_t* key_mask, int32_t B, int32_t S, const void* tape,
                            const float* d_out, float* const* grads, int32_t accumulate, void* workspace,
                            size_t workspace_bytes, void* stream);
int32_t m2_debug_encoder_grad_plan(int32_t V, int32_t H, int32_t layers, int32_t heads, int32_t B, int32_t S, char* out,
                                   size_t cap);
size_t m2_embedding_backward_workspace_bytes(int32_t R, int32_t V, int32_t H);
int32_t m2_embedding_backward(const int64_t* ids, const float* d_x, int32_t R, int32_t V, int32_t H, float scale,
                              float* d_emb, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);
size_t m2_layer_norm_backward_workspace_bytes(int32_t R, int32_t K);
int32_t m2_layer_norm_backward(const float* g_y, const float* x, const float* gamma, const float* g_res, int32_t R,
                               int32_t K, float* g_x, float* dgamma, float* dbeta, void* workspace,
                               size_t workspace_bytes, void* stream);
int32_t m2_length_regulator_backward(const float* d_reg, const int32_t* cum, int32_t B, int32_t S, int32_t H,
                                     int32_t T_out, float* d_enc, void* stream);

/* ---- the duration predictor's training forward and backward ----------------
 * DurationPredictor from its raw parameters, as the encoder above.  params: 10
 * device pointers in parameters() order: (conv.weight [H,H,3], conv.bias [H],
 * norm.weight [H], norm.bias [H]) of the two ConvBlocks, projection.weight
 * [1,H,1], projection.bias [1].  bn: 8 vectors [H] in one array [8,H], block by
 * block: alpha = gamma / sqrt(running_var + eps), beta' = beta - running_mean
 * alpha (the eval-mode BatchNorm as the affine of m2_conv1d), running_mean,
 * invstd = 1 / sqrt(running_var + eps).  The running statistics are constants:
 * they get no gradient and nothing writes them; no dropout.  The dimension
 * arguments are (H, B, S); enc is [B,S,H].  Supported: kernel size 3, H a
 * multiple of 8 from 16 to 128, S <= 2^20, B S <= 2^24, B H S <= 2^30 (else M2_E_SHAPE; the
 * _bytes queries return 0).  B = 0 or S = 0: nothing to do, M2_OK.
 *
 * m2_duration_train_forward: dur [B,S], bit-equal to the stand-alone module's
 * forward (m2_conv1d with the affine and ReLU twice, the first reading enc
 * transposed, then the k = 1 projection with softplus), the two blocks writing
 * into the tape: y1, y2 [B,H,S], post-ReLU.  m2_duration_tape_map(index = 0, 1)
 * names a map's offset (in floats) and its channel count.  The conv outputs u
 * are not kept: the backward recomputes them with the same conv launch.
 *
 * m2_duration_backward: given d_dur [B,S]: d_enc [B,S,H] (or NULL) and grads
 * (10 pointers, NULL skips, accumulate adds with one fp32 addition per
 * element).  d gamma is formed per element from u, so it is right where gamma
 * is 0 or negative.  No floating-point atomics: equal inputs give equal bits,
 * and d_enc of an utterance does not depend on the rest of the batch.  A short
 * workspace, and a short tape in m2_duration_train_forward, is M2_E_ARG;
 * m2_duration_backward takes no tape size: the tape must be the one the forward
 * of this shape filled (m2_duration_tape_bytes), which is the caller's to keep.
 *
 * m2_debug_duration_grad_plan: as m2_debug_decoder_grad_plan (the format is in
 * csrc/duration_grad_plan.h). */
size_t m2_duration_tape_bytes(int32_t H, int32_t B, int32_t S);
int32_t m2_duration_tape_map(int32_t H, int32_t B, int32_t S, int32_t index, size_t* offset_floats, int32_t* width);
int32_t m2_duration_train_forward(const float* const* params, const float* bn, int32_t H, const float* enc, int32_t B,
                                  int32_t S, float* dur, void* tape, size_t tape_bytes, void* stream);
size_t m2_duration_backward_workspace_bytes(int32_t H, int32_t B, int32_t S);
int32_t m2_duration_backward(const float* const* params, const float* bn, int32_t H, const float* enc, int32_t B,
                             int32_t S, const void* tape, const float* d_dur, float* d_enc, float* const* grads,
                             int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);
int32_t m2_debug_duration_grad_plan(int32_t H, int32_t B, int32_t S, char* out, size_t cap);

/* ---- measurement ----------------------------------------------------------
 * Kernel timing with HIP events recorded on the launch stream around each of
 * the fused vocoder's kernels (bench.py's roofline).  enable: allocate event
 * pairs for `capacity` m2_vocoder calls (outside any timed region); each call
 * then records one pair per kernel while capacity lasts.  read: synchronise
 * and return durations in ms, call-major ([call][kernel]), n_out = count, and
 * reset.  Kernels are named by m2_profile_kernel_name(i), i < count(). */
int32_t m2_profile_enable(m2_model* model, int32_t capacity);
int32_t m2_profile_read(m2_model* model, float* ms_out, int32_t capacity, int32_t* n_out);
int32_t m2_profile_disable(m2_model* model);
/* Record event pairs only around the kernels whose bit is set (default all);
 * m2_profile_read reports -1 for the others.  Every recorded event costs a
 * few microseconds of pipeline drain between kernels. */
int32_t m2_profile_select(m2_model* model, uint32_t kernel_mask);
/* Record on every `stride`-th m2_vocoder call only (default 1; the calls in
 * between record nothing and take no capacity), so a timed region can carry a
 * sample of the launches at a fraction of the event cost.  Reset by enable. */
int32_t m2_profile_stride(m2_model* model, int32_t stride);
int32_t m2_profile_kernel_count(void);
const char* m2_profile_kernel_name(int32_t index);
/* The same kernel as launched by this model (symbol prefix = rocprofv3 name). */
const char* m2_profile_kernel_name_for(const m2_model* model, int32_t index);
/* The launch plan of m2_vocoder(model, mel[B, T], mel_layout) as one line of
 * text: the path (perlayer | split | f32) and every launch with its variant,
 * grid, threads and LDS bytes, e.g.
 *   split stage=1 headmid[n=2 S=126 nch=8 trans=1 grid=2x3 thr=1024 lds=...]
 *   tailp[nl=6 nch=8 grid=4x3 thr=448 lds=49184] redo=none
 * (one line; the format is fixed and documented in csrc/vocoder_launch.h).
 * device_T != 0: as a speculative launch whose frame count is a device word.
 * Host arithmetic only: nothing is launched.  Writes at most cap bytes
 * (NUL-terminated) and returns the line's length, or a negative M2_E_* code. */
int32_t m2_debug_vocoder_plan(const m2_model* model, int32_t B, int32_t T, int32_t mel_layout, int32_t device_T,
                              char* out, size_t cap);
/* The device's workgroup slots (CUs x occupancy) that the plan's rules weigh,
 * queried once: the split-f16 stage2 heads of 16 / 19 / 24 / 27 frames, the
 * stage2 mid and its small-grid form, the stage2 tail and its small-grid form. */
int32_t m2_debug_vocoder_slots(int64_t* out8);
/* Vocoder arithmetic of this model: 0 per-layer fp32 kernels, 1 fused exact-f32
 * MFMA (v_mfma_f32_16x16x4_f32), 2 fused split-f16 MFMA (fp32 operands as
 * f16 hi/lo pairs, 3 products per fp32 product, fp32 accumulation). */
int32_t m2_vocoder_path(const m2_model* model);
/* Transformer arithmetic of this model: 1 = fused split-f16 layers and
 * attention, 2 = the same with at least one layer whose attention-score bound
 * reaches the f16 maximum (that layer keeps its softmax base in fp32 in every
 * attention form), 0 = fp32 linears and the exact-f32 attention (weights
 * whose activation bound leaves the f16 range, or M2_TF_UNFUSED / M2_ATT_F32
 * set when the handle is created: M2_ATT_F32 selects exactly what the range
 * bound selects, M2_TF_UNFUSED the fp32 linears with the default attention). */
int32_t m2_transformer_path(const m2_model* model);
/* The driver a call made now would run the layers of a stack on (stack: 0 text
 * encoder, 1 mel decoder), under the developer switches in force: 0 = five
 * fp32 linears per layer, 1 = three launches per layer, each LN1 -> QKV its
 * own launch (M2_TF_CHAIN=0), 2 = three launches per layer with the next
 * layer's LN1 -> QKV (or the final LN -> mel projection) chained into
 * post_attn_kernel, 3 = one launch per layer (transformer_layer.hip).  A stack
 * without layers reports the form its layers would take.  Host arithmetic on
 * the predicates the drivers branch on: nothing is launched.  Negative
 * M2_E_ARG for a null model or another stack. */
int32_t m2_debug_transformer_form(const m2_model* model, int32_t stack);
/* The launch plan of one forward of a stack (0 text encoder, 1 mel decoder) on
 * [B, N] rows as one line of text: the form above, then every launch in order
 * with its tile geometry, e.g.
 *   dec form=3 H=64 heads=2 layers=4 B=3 N=21 src=x masked=0 devT=0 ragged=0
 *   projected=1 tfl_first0[rb=1 grid=12 thr=512] tfl_layer0[next=1 rb=1
 *   qs2=12 grid=12 thr=512] ...
 * or error="<text>" where the call would be refused (one line; the format is
 * fixed and documented in csrc/transformer_plan.h).  masked: lengths are
 * given; source: 0 rows as given, 1 the embedding, 2 the length regulator's
 * frame expansion; device_T: N is the capacity of a speculative launch;
 * ragged: per-utterance row counts.  Only the calls an entry point makes
 * are planned (encoder: source 0 or 1, masked; decoder: source 0 or 2,
 * device_T, ragged), any other is M2_E_ARG.  Host arithmetic only: nothing is
 * launched.  Writes at most cap bytes (NUL-terminated) and returns the line's
 * length, or a negative M2_E_* code. */
int32_t m2_debug_transformer_plan(const m2_model* model, int32_t stack, int32_t B, int32_t N, int32_t masked,
                                  int32_t source, int32_t device_T, int32_t ragged, char* out, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* M2TTS_HIP_H */
