#!/usr/bin/env python3
"""Time the training losses on the GPU with HIP events.

    python tools/time_losses.py [--batch 32] [--length 32000] [--frames 500] [--mels 64] [--phonemes 100]

Prints one JSON line: milliseconds per CombinedTTSLoss call in generator and in
discriminator mode, per spectral / discriminator part, and for the two heaviest
packed layers of scale 1 (the grouped 64 -> 128 k = 41 stride-4 layer and the
dense 1024 -> 1024 k = 5 layer) their time and FLOP/time as a fraction of the
fp32 MFMA peak (157.3 TFLOP/s).  The discriminator step (enable_backward():
the discriminator loss forward and backward, m2_disc_step) is timed as
discriminator_loss(...).backward() against the forward-only discriminator_loss
call of the same process (step_over_forward), and the two MFMA gradients of the
same two layers on their own: the weight gradient (its split-K kernel and the
fixed-order finish), and the data gradient as the difference between a call
that computes both and one that computes the weight gradient alone.  The
generator step is the generator-mode call again with the three predictions
requiring grad (generator_step_ms, against generator_ms: generator_step_over_forward),
generator_terms(...).backward(), m2_disc_gen_step alone, and the first-layer
audio gradient kernel summed over the three scales.  The spectral switch
(enable_backward(spectral=True)): the generator-mode call alone
(generator_spectral_call_ms), the call with total_loss.backward()
(generator_spectral_step_ms, against generator_step_ms), and the three
m2_loss_spectral_backward calls of the default weights on their own
(spectral_backward_ms, against spectral_and_perceptual_ms:
spectral_backward_over_forward).  The vocoder's training side (DESIGN 4.6d,
stage1 vocoder, --frames frames): m2_vocoder_train_forward
(vocoder_train_forward_ms), m2_vocoder_backward with every parameter gradient
(vocoder_backward_ms, against the forward: vocoder_backward_over_forward), and
the generator-mode call on audio_pred = vocoder(mel) with total_loss.backward()
reaching the vocoder's parameters (gen_step_vocoder_ms; only when --length is
64 x --frames).  The mel decoder's training side (--hidden,
--dec-layers, --heads, default the stage1 decoder): m2_decoder_train_forward
(decoder_train_forward_ms), m2_decoder_backward with every gradient and d_x
(decoder_backward_ms, decoder_backward_over_forward), and the same generator
step with mel = decoder(x) feeding both the mel loss and the vocoder
(gen_step_decoder_ms, under gen_step_vocoder_ms's condition).  --decoder-only
prints the two decoder lines alone (for a kernel trace).  The text
encoder's training side and the length regulator's adjoint (DESIGN 4.6f;
--vocab, --hidden, --enc-layers, --heads, --phonemes, default the stage1
encoder at 100 phonemes): --encoder-only prints m2_encoder_train_forward
(encoder_train_forward_ms), m2_encoder_backward with every gradient
(encoder_backward_ms, encoder_backward_over_forward) and
m2_length_regulator_backward at --frames frames per utterance
(regulator_adjoint_ms), alone.  The duration predictor's training side
(--hidden, --phonemes): --duration-only prints
m2_duration_train_forward (duration_train_forward_ms) and m2_duration_backward
with every gradient and d_enc (duration_backward_ms,
duration_backward_over_forward), alone.  --model-step prints the stage-1
training step of an M2TTSModel with enable_backward() in training mode, at
--phonemes phonemes and --frames frames per utterance: forward with a graph
(model_forward_graph_ms), then the same plus the reference's stage-1 loss
(L1 mel + 0.1 x MSE duration) and backward() (model_step_ms), alone.  Each
figure is the median of --iters timed calls after --warmup untimed ones.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "m2-tts_amd" / "src"))

PEAK_F32_MFMA = 157.3e12


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def decoder_lines(out, args, dev):
    """The mel decoder's training forward and backward; returns the module, its input and its
    parameters."""
    from m2amd import ops
    from models.tts_model import MelDecoder
    dec = MelDecoder(args.hidden, args.mels, args.dec_layers, args.heads).to(dev).enable_backward()
    params = [p.detach() for p in dec.parameters()]
    x = torch.randn(args.batch, args.frames, args.hidden, device=dev)
    _, tape = ops.decoder_train_forward(params, x, args.heads)
    d_mel = torch.randn(args.batch, args.frames, args.mels, device=dev)
    out["decoder_train_forward_ms"] = timed(lambda: ops.decoder_train_forward(params, x, args.heads), args.warmup,
                                            args.iters)
    out["decoder_backward_ms"] = timed(lambda: ops.decoder_backward(params, x, tape, d_mel, args.heads), args.warmup,
                                       args.iters)
    out["decoder_backward_over_forward"] = out["decoder_backward_ms"] / out["decoder_train_forward_ms"]
    return dec, x


def encoder_lines(out, args, dev):
    """The text encoder's training forward and backward and the length regulator's adjoint."""
    from m2amd import ops
    from models.tts_model import TextEncoder
    B, S, T, H = args.batch, args.phonemes, args.frames, args.hidden
    enc = TextEncoder(args.vocab, H, args.enc_layers, args.heads).to(dev)
    params = [p.detach() for p in enc.parameters()]
    pe = enc.pos_encoding.pe[0]
    ids = torch.randint(0, args.vocab, (B, S), device=dev)
    mask = torch.arange(S, device=dev)[None, :] < torch.randint(S // 2, S + 1, (B, 1), device=dev)
    _, tape = ops.encoder_train_forward(params, ids, pe, mask, args.heads)
    d_out = torch.randn(B, S, H, device=dev)
    out["encoder_train_forward_ms"] = timed(lambda: ops.encoder_train_forward(params, ids, pe, mask, args.heads),
                                            args.warmup, args.iters)
    out["encoder_backward_ms"] = timed(lambda: ops.encoder_backward(params, ids, mask, tape, d_out, args.heads),
                                       args.warmup, args.iters)
    out["encoder_backward_over_forward"] = out["encoder_backward_ms"] / out["encoder_train_forward_ms"]
    # every utterance fills its T frames: T // S per phoneme and the remainder on the first ones
    durations = torch.full((B, S), T // S, dtype=torch.int64, device=dev)
    durations[:, :T % S] += 1
    cum, _, _ = ops.frame_counts(durations)
    d_reg = torch.randn(B, T, H, device=dev)
    out["regulator_adjoint_ms"] = timed(lambda: ops.regulate_backward(d_reg, cum, S), args.warmup, args.iters)


def duration_lines(out, args, dev):
    """The duration predictor's training forward and backward."""
    from m2amd import ops
    from models.tts_model import DurationPredictor
    B, S, H = args.batch, args.phonemes, args.hidden
    pred = DurationPredictor(H).to(dev).eval()
    params = [p.detach() for p in pred.parameters()]
    bn = torch.cat([ops.batchnorm_eval_stats(b.norm.weight, b.norm.bias, b.norm.running_mean, b.norm.running_var,
                                             b.norm.eps) for b in pred.predictor.conv_layers])
    enc = torch.randn(B, S, H, device=dev)
    _, tape = ops.duration_train_forward(params, bn, enc)
    d_dur = torch.randn(B, S, device=dev)
    out["duration_train_forward_ms"] = timed(lambda: ops.duration_train_forward(params, bn, enc), args.warmup,
                                             args.iters)
    out["duration_backward_ms"] = timed(lambda: ops.duration_backward(params, bn, enc, tape, d_dur), args.warmup,
                                        args.iters)
    out["duration_backward_over_forward"] = out["duration_backward_ms"] / out["duration_train_forward_ms"]


def model_step_lines(out, args, dev):
    """M2TTSModel.forward with a graph, and the stage-1 step: the reference's loss (L1 mel + 0.1 x MSE
    duration) and backward().  Every utterance fills its --frames frames."""
    import warnings

    import torch.nn.functional as F
    from models.tts_model import M2TTSModel
    B, S, T, H, M = args.batch, args.phonemes, args.frames, args.hidden, args.mels
    model = M2TTSModel(args.vocab, H, M, args.enc_layers, args.dec_layers, args.heads).to(dev).train().enable_backward()
    ids = torch.randint(0, args.vocab, (B, S), device=dev)
    lengths = torch.randint(S // 2, S + 1, (B,), device=dev)
    durations = torch.full((B, S), T // S, dtype=torch.int64, device=dev)
    durations[:, :T % S] += 1
    target = torch.randn(B, T, M, device=dev)

    def forward():
        return model(ids, lengths, target_durations=durations, max_target_length=T)

    def step():
        for p in model.parameters():
            p.grad = None
        o = forward()
        (F.l1_loss(o["mel_output"], target) + 0.1 * F.mse_loss(o["duration_pred"], durations.float())).backward()

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # training mode computes the eval function, said once
        out["model_forward_graph_ms"] = timed(forward, args.warmup, args.iters)
        out["model_step_ms"] = timed(step, args.warmup, args.iters)
    out["model_step_over_forward"] = out["model_step_ms"] / out["model_forward_graph_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--length", type=int, default=32000)
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--mels", type=int, default=64)
    ap.add_argument("--phonemes", type=int, default=100)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--dec-layers", type=int, default=2)
    ap.add_argument("--heads", type=int, default=2)
    ap.add_argument("--decoder-only", action="store_true")
    ap.add_argument("--vocab", type=int, default=256)
    ap.add_argument("--enc-layers", type=int, default=2)
    ap.add_argument("--encoder-only", action="store_true")
    ap.add_argument("--duration-only", action="store_true")
    ap.add_argument("--model-step", action="store_true")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()

    from training.losses import CombinedTTSLoss
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    if args.decoder_only:
        out = {"batch": args.batch, "frames": args.frames, "mels": args.mels, "hidden": args.hidden,
               "dec_layers": args.dec_layers, "heads": args.heads, "iters": args.iters}
        decoder_lines(out, args, dev)
        print(json.dumps(out))
        return
    if args.encoder_only:
        out = {"batch": args.batch, "phonemes": args.phonemes, "frames": args.frames, "vocab": args.vocab,
               "hidden": args.hidden, "enc_layers": args.enc_layers, "heads": args.heads, "iters": args.iters}
        encoder_lines(out, args, dev)
        print(json.dumps(out))
        return
    if args.duration_only:
        out = {"batch": args.batch, "phonemes": args.phonemes, "hidden": args.hidden, "iters": args.iters}
        duration_lines(out, args, dev)
        print(json.dumps(out))
        return
    if args.model_step:
        out = {"batch": args.batch, "phonemes": args.phonemes, "frames": args.frames, "mels": args.mels,
               "vocab": args.vocab, "hidden": args.hidden, "enc_layers": args.enc_layers, "dec_layers": args.dec_layers,
               "heads": args.heads, "iters": args.iters}
        model_step_lines(out, args, dev)
        print(json.dumps(out))
        return
    loss = CombinedTTSLoss().eval().to(dev)
    B, L, T, M, S = args.batch, args.length, args.frames, args.mels, args.phonemes
    kw = dict(mel_pred=torch.randn(B, T, M, device=dev), mel_target=torch.randn(B, M, T, device=dev),
              duration_pred=torch.rand(B, S, device=dev) + 0.5, duration_target=torch.rand(B, S, device=dev) + 0.5,
              audio_target=torch.tanh(torch.randn(B, 1, L, device=dev)),
              mel_lengths=torch.full((B,), T, device=dev))
    kw["audio_pred"] = torch.tanh(torch.atanh(kw["audio_target"] * 0.999) + 0.1 * torch.randn(B, 1, L, device=dev))
    out = {"batch": B, "length": L, "frames": T, "mels": M, "phonemes": S, "iters": args.iters}
    out["generator_ms"] = timed(lambda: loss(**kw, optimize_discriminator=False), args.warmup, args.iters)
    out["discriminator_ms"] = timed(lambda: loss(**kw, optimize_discriminator=True), args.warmup, args.iters)
    out["spectral_and_perceptual_ms"] = timed(
        lambda: (loss.spectral_loss(kw["audio_pred"], kw["audio_target"]),
                 loss.perceptual_loss(kw["audio_pred"], kw["audio_target"])), args.warmup, args.iters)
    disc = loss.adversarial_loss.discriminator
    out["discriminator_sums_ms"] = timed(lambda: disc._sums(kw["audio_target"], kw["audio_pred"]), args.warmup,
                                         args.iters)
    adv = loss.adversarial_loss
    real, fake = kw["audio_target"], kw["audio_pred"]
    out["discriminator_loss_forward_ms"] = timed(lambda: adv.discriminator_loss(real, fake), args.warmup, args.iters)
    loss.enable_backward()

    def step():
        for p in disc.parameters():
            p.grad = None
        adv.discriminator_loss(real, fake).backward()

    out["discriminator_step_ms"] = timed(step, args.warmup, args.iters)
    loss.enable_backward(False)
    for p in disc.parameters():
        p.grad = None
    out["step_over_forward"] = out["discriminator_step_ms"] / out["discriminator_loss_forward_ms"]
    h = disc._handle(dev)
    # the generator step: the same generator-mode call with the predictions requiring grad (one
    # m2_disc_gen_step instead of m2_disc_losses, the mel and duration gradients), against generator_ms above
    loss.enable_backward()
    kg = dict(kw)
    for k in ("mel_pred", "duration_pred", "audio_pred"):
        kg[k] = kw[k].clone().requires_grad_()

    def gen_step():
        kg["audio_pred"].grad = None
        adv.generator_terms(real, kg["audio_pred"], loss.adversarial_loss_weight,
                            loss.feature_matching_weight).backward()

    out["generator_step_ms"] = timed(lambda: loss(**kg, optimize_discriminator=False), args.warmup, args.iters)
    out["generator_step_over_forward"] = out["generator_step_ms"] / out["generator_ms"]
    out["generator_terms_backward_ms"] = timed(gen_step, args.warmup, args.iters)
    # the spectral switch: the same call (its spectral gradient is computed in backward, so the call
    # alone costs what generator_step_ms does), the call with total_loss.backward(), and the three
    # m2_loss_spectral_backward calls alone against the forward line spectral_and_perceptual_ms
    from training.losses import _spectral_gradient, spectral_backward_calls
    loss.enable_backward(spectral=True)

    def spectral_step():
        for k in ("mel_pred", "duration_pred", "audio_pred"):
            kg[k].grad = None
        loss(**kg, optimize_discriminator=False)["total_loss"].backward()

    out["generator_spectral_call_ms"] = timed(lambda: loss(**kg, optimize_discriminator=False), args.warmup, args.iters)
    out["generator_spectral_step_ms"] = timed(spectral_step, args.warmup, args.iters)
    out["generator_spectral_step_over_generator_step"] = out["generator_spectral_step_ms"] / out["generator_step_ms"]
    calls = spectral_backward_calls(B, L, loss.spectral_loss.n_fft_list, loss.spectral_loss.hop_length_factor,
                                    loss.spectral_loss_weight, loss.perceptual_loss_weight)
    out["spectral_backward_ms"] = timed(lambda: _spectral_gradient(fake, real, calls), args.warmup, args.iters)
    out["spectral_backward_over_forward"] = out["spectral_backward_ms"] / out["spectral_and_perceptual_ms"]
    loss.enable_backward(False)
    out["gen_step_ms"] = timed(lambda: h.gen_step(real, fake, loss.adversarial_loss_weight,
                                                  loss.feature_matching_weight), args.warmup, args.iters)
    from m2amd import ops
    w0 = disc.discriminators[0][0].weight.detach()
    audio_ms = 0.0
    for pool in disc.scales:  # the first-layer data gradient down to the samples, once per scale as in the step
        dy0 = torch.randn(B, 64, L // pool, device=dev)
        audio_ms += timed(lambda: ops.conv1d_audio_backward(dy0, w0, L, padding=7, pool=pool), args.warmup, args.iters)
    out["audio_gradient_ms"] = audio_ms
    out["audio_gradient_share_of_gen_step"] = audio_ms / out["gen_step_ms"]
    shapes = h.shapes(L)[0]
    for name, layer in (("grouped_64_128_k41", 1), ("dense_1024_1024_k5", 5)):
        cin, cout, k, _, _, groups = h.LAYER_TABLE[layer]
        x = torch.randn(B, cin, shapes[layer - 1][1], device=dev)
        ms = timed(lambda: h.layer(0, layer, x), args.warmup, args.iters)
        flop = 2.0 * cout * (cin // groups) * k * shapes[layer][1] * B
        out[name] = {"ms": ms, "gflop": flop / 1e9, "fraction_of_f32_mfma_peak": flop / (ms * 1e-3) / PEAK_F32_MFMA}
        from m2amd import ops
        _, _, _, stride, pad, _ = h.LAYER_TABLE[layer]
        w = torch.randn(cout, cin // groups, k, device=dev)
        dy = torch.randn(B, cout, shapes[layer][1], device=dev)
        geo = dict(stride=stride, padding=pad, groups=groups, in_slope=0.2, need_db=False)
        dw_ms = timed(lambda: ops.conv1d_strided_backward(x, w, dy, need_dx=False, **geo), args.warmup, args.iters)
        both_ms = timed(lambda: ops.conv1d_strided_backward(x, w, dy, need_dx=True, **geo), args.warmup, args.iters)
        for key, t in (("weight_gradient", dw_ms), ("data_gradient", both_ms - dw_ms)):
            out[name][key] = {"ms": t, "fraction_of_f32_mfma_peak": flop / (t * 1e-3) / PEAK_F32_MFMA}
    # the vocoder's training forward and backward on the stage1 vocoder, and the generator-mode
    # call with total_loss.backward() reaching the vocoder's parameters through audio_pred = vocoder(mel)
    from models.tts_model import SimpleVocoder
    voc = SimpleVocoder(mel_channels=M).to(dev).enable_backward()
    vparams = [p.detach() for p in voc.parameters()]
    vmel = torch.randn(B, M, T, device=dev)
    _, tape = ops.vocoder_train_forward(vparams, vmel)
    d_audio = torch.randn(B, 1, 64 * T, device=dev)
    out["vocoder_train_forward_ms"] = timed(lambda: ops.vocoder_train_forward(vparams, vmel), args.warmup, args.iters)
    out["vocoder_backward_ms"] = timed(lambda: ops.vocoder_backward(vparams, vmel, tape, d_audio, need_mel=False),
                                       args.warmup, args.iters)
    out["vocoder_backward_over_forward"] = out["vocoder_backward_ms"] / out["vocoder_train_forward_ms"]
    if L == 64 * T:
        loss.enable_backward(spectral=True)
        kv = {k: v for k, v in kg.items() if k != "audio_pred"}  # mel and duration predictions require grad

        def vocoder_step():
            for p in voc.parameters():
                p.grad = None
            for k in ("mel_pred", "duration_pred"):
                kg[k].grad = None
            loss(audio_pred=voc(vmel), **kv, optimize_discriminator=False)["total_loss"].backward()

        out["gen_step_vocoder_ms"] = timed(vocoder_step, args.warmup, args.iters)
        loss.enable_backward(False)
    dec, dx = decoder_lines(out, args, dev)
    if L == 64 * T:
        loss.enable_backward(spectral=True)
        kd = {k: v for k, v in kg.items() if k not in ("audio_pred", "mel_pred")}
        dx.requires_grad_()

        def decoder_step():
            for p in list(voc.parameters()) + list(dec.parameters()) + [dx, kg["duration_pred"]]:
                p.grad = None
            mel = dec(dx)
            loss(mel_pred=mel, audio_pred=voc(mel.transpose(1, 2)), **kd,
                 optimize_discriminator=False)["total_loss"].backward()

        out["gen_step_decoder_ms"] = timed(decoder_step, args.warmup, args.iters)
        loss.enable_backward(False)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
