"""GPU: M2TTSModel.forward with a graph (M2TTSModel.enable_backward) and the
reference trainer's stage-1 step written out by hand: an L1 mel loss plus 0.1 x
an MSE duration loss formed with torch's own ops, backward(), clip_grad_norm_
and an SGD step, against the float64 chain text encoder -> duration predictor
-> length regulator (index arithmetic) -> mel decoder of
tests/golden/{encoder,duration,decoder}_backward_oracle.py.  Nothing here
reads the reference.

The stage-1 model (stage_config) with the golden stage-1 weights and
non-degenerate BatchNorm statistics, B = 2, S = 9, lengths (9, 6), integer
target durations in 0..3 with zeros.

The bar is test_gpu_encoder_backward.py's: per tensor
    |g_gpu - g_f64| <= 32 x max(s, 2^-24) x max|g_f64|,
s the largest relative deviation of CPU float32 autograd from float64 over the
step's tensors, computed here and printed; ReLU predicates come from the GPU's
tapes, a differing one must lie within the forward bar of its map, at most 4
may differ.

The clipped step.  clip_grad_norm_ scales every gradient by c = 1 / (n + 1e-6),
n the norm over all gradients (when n > 1).  Each tensor's error is at most
bar x max|g_i| per element, so the norm's is at most bar x N, N = sqrt(sum_i
numel_i max|g_i|^2), and c's relative error at most r = bar N / n + 8 x 2^-24
(the float32 norm's own rounding).  A parameter after the step may therefore
differ from the float64 step by lr c max|g| (bar + r (1 + bar)) + 2^-24 max|p|.
"""
import copy
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, MEL_MAXABS_TOL, golden_state, maxabs, stage_config

sys.path.insert(0, str(GOLDEN))
import decoder_backward_oracle as dorc  # noqa: E402
import duration_backward_oracle as uorc  # noqa: E402
import encoder_backward_oracle as eorc  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
ENC_TOL = 1e-4  # test_gpu_parity.py's bar for the intermediate tensors
KINK_CAP = 4
LR = 0.05
B, S, H, M, HEADS, LAYERS = 2, 9, 64, 64, 2, 2
KEYS = ["encoder_output", "duration_pred", "regulated_output", "mel_output", "audio_output", "padding_mask"]
DUR = [[2, 0, 3, 1, 2, 1, 3, 1, 2], [1, 3, 0, 2, 0, 1, 0, 0, 0]]


def _rel(a, b):
    return float((a.double() - b).abs().max()) / float(b.abs().max())


def _new_model(gpu):
    from models.tts_model import M2TTSModel
    torch.manual_seed(51)
    model = M2TTSModel(**stage_config("s1").as_dict())
    model.load_state_dict(golden_state("s1"))
    uorc.randomize_norms(model.duration_predictor, 51)
    return model.to(gpu).eval()


def _inputs(gpu):
    g = torch.Generator().manual_seed(52)
    ids = torch.randint(0, 256, (B, S), generator=g)
    lengths = torch.tensor([9, 6])
    dur = torch.tensor(DUR)
    assert dur.shape == (B, S) and int(dur.min()) == 0 and int(dur.max()) == 3
    T = int(dur.sum(1).max())
    target = torch.randn(B, T, M, generator=g)
    return {"ids": ids.to(gpu), "lengths": lengths.to(gpu), "dur": dur.to(gpu), "target": target.to(gpu), "T": T,
            "ids_c": ids, "lengths_c": lengths, "dur_c": dur, "target_c": target}


def _loss(mel, target, dur_pred, durations):
    """The reference's TTSLoss: L1 on the mel plus 0.1 x MSE on the durations (durations.float() on the GPU;
    the float64 chain keeps its own precision)."""
    return F.l1_loss(mel, target) + 0.1 * F.mse_loss(dur_pred, durations.to(dur_pred.dtype))


def _trainable(model):
    return (list(model.text_encoder.parameters()) + list(model.duration_predictor.parameters())
            + list(model.decoder.parameters()))


def _bn_stats(pred):
    from m2amd import ops
    return torch.cat([ops.batchnorm_eval_stats(b.norm.weight, b.norm.bias, b.norm.running_mean, b.norm.running_var,
                                               b.norm.eps) for b in pred.predictor.conv_layers])


def test_flag_off_is_todays_forward(gpu):
    model, x = _new_model(gpu), _inputs(gpu)
    args = (x["ids"], x["lengths"])
    kw = dict(target_durations=x["dur"], max_target_length=x["T"])
    before = model(*args, **kw)  # before enable_backward was ever touched
    assert list(before) == KEYS and all(v.grad_fn is None for v in before.values())
    assert model.backward_enabled is False
    model.enable_backward()
    model.enable_backward(False)
    for out in (model(*args, **kw), ):
        assert list(out) == KEYS and all(v.grad_fn is None and torch.equal(v, before[k]) for k, v in out.items())
    model.enable_backward()
    with torch.no_grad():  # on, but gradients are disabled: the handle
        out = model(*args, **kw)
    assert all(v.grad_fn is None and torch.equal(v, before[k]) for k, v in out.items())
    for p in model.parameters():
        p.requires_grad_(False)
    out = model(*args, **kw)  # on, but nothing requires grad
    assert all(v.grad_fn is None and torch.equal(v, before[k]) for k, v in out.items())
    free = model(*args)  # predicted durations, no target
    model.enable_backward(False)
    assert all(torch.equal(v, w) for v, w in zip(free.values(), model(*args).values()))


def test_flag_on_composes_the_stage_modules(gpu):
    model, x = _new_model(gpu), _inputs(gpu)
    handle = model(x["ids"], x["lengths"], target_durations=x["dur"], max_target_length=x["T"])
    model.train()
    assert model.enable_backward() is model
    with pytest.warns(RuntimeWarning):  # the eval function is computed; said once per module class
        from models import components
        components._WARNED.clear()
        out = model(x["ids"], x["lengths"], target_durations=x["dur"], max_target_length=x["T"])
    assert list(out) == KEYS and out["audio_output"] is None
    assert out["mel_output"].grad_fn is not None and out["duration_pred"].grad_fn is not None
    assert out["encoder_output"].grad_fn is not None and out["regulated_output"].grad_fn is not None
    assert out["mel_output"].shape == (B, x["T"], M) and out["duration_pred"].shape == (B, S)
    # the stage modules one by one, their switches on
    enc, mask = model.text_encoder(x["ids"], x["lengths"])
    dur = model.duration_predictor(enc)
    reg = model.length_regulator(enc, x["dur"], x["T"])
    mel = model.decoder(reg)
    for k, v in (("encoder_output", enc), ("duration_pred", dur), ("regulated_output", reg), ("mel_output", mel),
                 ("padding_mask", mask)):
        assert torch.equal(out[k].detach(), v.detach()), k
    # and today's forward within the parity bars
    assert torch.equal(out["padding_mask"], handle["padding_mask"])
    for k in ("encoder_output", "duration_pred", "regulated_output"):
        assert out[k].shape == handle[k].shape and maxabs(out[k].detach(), handle[k]) <= ENC_TOL, k
    assert maxabs(out["mel_output"].detach(), handle["mel_output"]) <= MEL_MAXABS_TOL
    model.enable_backward(False).eval()


def _ops_step(model, x, with_duration_term=True, target_durations=True):
    """The step as an ops-level composition: (the gradients of the text encoder's, the duration predictor's and
    the decoder's parameters, the tapes and what the float64 chain needs)."""
    from m2amd import ops
    ep = [p.detach() for p in model.text_encoder.parameters()]
    up = [p.detach() for p in model.duration_predictor.parameters()]
    dp = [p.detach() for p in model.decoder.parameters()]
    bn = _bn_stats(model.duration_predictor)
    mask = eorc.key_mask(x["lengths_c"], S).to(x["ids"].device)
    enc, tape_e = ops.encoder_train_forward(ep, x["ids"], model.text_encoder.pos_encoding.pe[0], mask, HEADS)
    dur, tape_u = ops.duration_train_forward(up, bn, enc)
    durations = x["dur"] if target_durations else dur
    reg, cum = ops.regulate_with_counts(enc, durations, x["T"] if target_durations else None)
    mel, tape_d = ops.decoder_train_forward(dp, reg, HEADS)
    mel_leaf, dur_leaf = mel.clone().requires_grad_(), dur.clone().requires_grad_()
    target = x["target"] if target_durations else torch.zeros_like(mel)
    loss = _loss(mel_leaf, target, dur_leaf, x["dur"]) if with_duration_term else F.l1_loss(mel_leaf, target)
    loss.backward()
    d_reg, dgrads = ops.decoder_backward(dp, reg, tape_d, mel_leaf.grad, HEADS)
    d_enc = d_enc_reg = ops.regulate_backward(d_reg, cum, S)
    d_enc_u, ugrads = None, [None] * 10
    if with_duration_term:
        d_enc_u, ugrads = ops.duration_backward(up, bn, enc, tape_u, dur_leaf.grad)
        d_enc = d_enc_u + d_enc_reg  # autograd's one addition
    egrads = ops.encoder_backward(ep, x["ids"], mask, tape_e, d_enc, HEADS)
    return {"grads": egrads + ugrads + dgrads, "enc": enc, "dur": dur, "reg": reg, "mel": mel, "cum": cum,
            "d_enc_parts": (d_enc_reg, d_enc_u), "encoder_args": (ep, x["ids"], mask, tape_e),
            "tapes": (tape_e, tape_u, tape_d), "g_mel": mel_leaf.grad, "g_dur": dur_leaf.grad, "loss": loss.detach()}


def _float64_step(model, x, step):
    """The float64 chain's gradients of the step's loss with the tapes' predicates, the bar, and the count of
    differing predicates."""
    from m2amd import ops
    tape_e, tape_u, tape_d = step["tapes"]
    T = x["T"]
    _, emaps = ops.encoder_tape_maps(tape_e, 256, H, LAYERS, HEADS, B, S)
    umaps = ops.duration_tape_maps(tape_u, H, B, S)
    dmaps = ops.decoder_tape_maps(tape_d, H, M, LAYERS, HEADS, B, T)
    pos_e, pos_d = [m["h"].cpu() > 0 for m in emaps], [m["h"].cpu() > 0 for m in dmaps]
    pos_u = [umaps["y1"].cpu() > 0, umaps["y2"].cpu() > 0]
    cum64 = eorc.frame_counts(x["dur_c"])
    assert torch.equal(step["cum"].cpu().to(torch.int64), cum64)

    def chain(dtype, pe_=None, pu_=None, pd_=None):
        e_ = eorc.cpu_copy(model.text_encoder, dtype)
        u_ = uorc.cpu_copy(model.duration_predictor, dtype)
        d_ = dorc.cpu_copy(model.decoder, dtype)
        enc, pre_e, _ = eorc.forward(e_, x["ids_c"], x["lengths_c"], pe_)
        dur, pre_u, _, _ = uorc.forward(u_, enc, pu_)
        mel, pre_d = dorc.forward(d_, eorc.regulate(enc, cum64, T), pd_)
        loss = _loss(mel, x["target_c"].to(dtype), dur, x["dur_c"].to(dtype))
        grads = torch.autograd.grad(loss, eorc.parameters(e_) + uorc.parameters(u_) + dorc.parameters(d_))
        return list(grads), [[a.detach() for a in pre] for pre in (pre_e, pre_u, pre_d)], loss.detach()

    g64, pre64, loss64 = chain(torch.float64)
    g32, pre32, _ = chain(torch.float32)
    want, pre, _ = chain(torch.float64, pos_e, pos_u, pos_d)
    kinks = 0
    for name, p, p32, p64, pos in zip(("encoder", "duration", "decoder"), pre, pre32, pre64, (pos_e, pos_u, pos_d)):
        for l in range(len(p)):
            top = float(p64[l].abs().max())
            s_fwd = float((p32[l].double() - p64[l]).abs().max()) / top
            differ = (p[l] > 0) != pos[l]
            assert bool((p[l].abs()[differ] <= 32.0 * max(s_fwd, EPS) * top).all()), (name, l)
            kinks += int(differ.sum())
    assert kinks <= KINK_CAP
    s = max(_rel(a, b) for a, b in zip(g32, g64) if float(b.abs().max()) > 0)
    assert abs(float(step["loss"]) - float(loss64)) <= 1e-5 * float(loss64)
    return want, 32.0 * max(s, EPS), s, kinks


def test_stage1_step(gpu):
    model, x = _new_model(gpu), _inputs(gpu)
    model.train().enable_backward()
    params = _trainable(model)
    names = [n for n, _ in model.named_parameters() if not n.startswith("vocoder.")]
    assert len(params) == len(names) == 25 + 10 + 26
    out = model(x["ids"], x["lengths"], target_durations=x["dur"], max_target_length=x["T"])
    loss = _loss(out["mel_output"], x["target"], out["duration_pred"], x["dur"])
    loss.backward()
    got = [p.grad.clone() for p in params]  # every one has a .grad
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in got)
    assert all(p.grad is None for p in model.vocoder.parameters())
    for blk in model.duration_predictor.predictor.conv_layers:
        assert int(blk.norm.num_batches_tracked) == 0 and not blk.norm.running_mean.requires_grad

    # the ops-level composition, bit for bit
    step = _ops_step(model, x)
    for k, v in (("encoder_output", "enc"), ("duration_pred", "dur"), ("regulated_output", "reg"), ("mel_output", "mel")):
        assert torch.equal(out[k].detach(), step[v]), k
    assert torch.equal(loss.detach(), step["loss"])
    for name, a, b in zip(names, got, step["grads"]):
        assert torch.equal(a, b), name

    # the float64 chain within the bar
    want, bar, s, kinks = _float64_step(model, x, step)
    worst = max(_rel(a.cpu(), b) for a, b in zip(got, want))
    print(f"stage-1 step: {kinks} kinks differ; worst rel max err {worst:.3e}, cpu float32 {s:.3e}, bar {bar:.3e}")
    for name, a, b in zip(names, got, want):
        assert a.shape == b.shape and _rel(a.cpu(), b) <= bar, (name, _rel(a.cpu(), b), bar)

    # the duration term arrives: the embedding's and the encoder's gradients are not the mel term's alone
    mel_only = _ops_step(model, x, with_duration_term=False)
    assert all(g is None for g in mel_only["grads"][25:35])
    assert all(not torch.equal(a, b) for a, b in zip(got[:25], mel_only["grads"][:25]))
    assert all(torch.equal(a, b) for a, b in zip(got[35:], mel_only["grads"][35:]))  # the decoder sees the mel term only

    # clip_grad_norm_ over the whole model and an SGD step, against float64
    before = [p.detach().clone() for p in params]
    voc_before = [p.detach().clone() for p in model.vocoder.parameters()]
    opt = torch.optim.SGD(model.parameters(), lr=LR)
    total = torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
    opt.step()
    p64 = [p.cpu().double().requires_grad_() for p in before]
    for p, g in zip(p64, want):
        p.grad = g.clone()
    n64 = float(torch.nn.utils.clip_grad_norm_(p64, 1.0))
    torch.optim.SGD(p64, lr=LR).step()
    c = min(1.0, 1.0 / (n64 + 1e-6))
    N = sum(g.numel() * float(g.abs().max()) ** 2 for g in want) ** 0.5
    r = bar * N / n64 + 8 * EPS
    print(f"clip: norm {n64:.4e} (float32 on the GPU {float(total):.4e}), coefficient {c:.4e}, r {r:.3e}")
    for name, p, q, g in zip(names, params, p64, want):
        err = float((p.detach().cpu().double() - q.detach()).abs().max())
        allow = LR * c * float(g.abs().max()) * (bar + r * (1 + bar)) + EPS * float(q.detach().abs().max())
        assert err <= allow, (name, err, allow)
    assert any(not torch.equal(p.detach(), b) for p, b in zip(params, before))
    assert all(torch.equal(p.detach(), b) for p, b in zip(model.vocoder.parameters(), voc_before))
    # the next forward reads the updated weights
    again = model(x["ids"], x["lengths"], target_durations=x["dur"], max_target_length=x["T"])
    assert not torch.equal(again["mel_output"].detach(), out["mel_output"].detach())
    fresh = _ops_step(model, x)
    assert torch.equal(again["mel_output"].detach(), fresh["mel"]) and torch.equal(again["duration_pred"].detach(), fresh["dur"])
    model.enable_backward(False).eval()


def test_predicted_durations_get_no_gradient_through_the_regulator(gpu):
    from m2amd import ops
    model, x = _new_model(gpu), _inputs(gpu)
    model.train().enable_backward()
    uparams = list(model.duration_predictor.parameters())
    out = model(x["ids"], x["lengths"])  # target_durations=None: the regulator sees dur.detach()
    dur = out["duration_pred"]
    assert dur.grad_fn is not None and out["mel_output"].grad_fn is not None
    assert torch.equal(out["regulated_output"].detach(), ops.regulate(out["encoder_output"].detach(), dur.detach()))
    T = out["mel_output"].shape[1]
    assert T == int(dur.detach().floor().clamp(min=0).sum(1).max()) and T > S
    # the mel term alone does not reach the predictor
    F.l1_loss(out["mel_output"], torch.zeros_like(out["mel_output"])).backward(retain_graph=True)
    assert all(p.grad is None for p in uparams)
    assert all(p.grad is not None for p in list(model.text_encoder.parameters()) + list(model.decoder.parameters()))
    # with its own term, the predictor's gradient is that term's alone
    (0.1 * F.mse_loss(dur, x["dur"].float())).backward()
    step = _ops_step(model, x, target_durations=False)
    assert torch.equal(step["dur"], dur.detach()) and torch.equal(step["mel"], out["mel_output"].detach())
    for p, g in zip(uparams, step["grads"][25:35]):
        assert torch.equal(p.grad, g)
    for p, g in zip(model.decoder.parameters(), step["grads"][35:]):
        assert torch.equal(p.grad, g)
    # The encoder's is the sum of both.  Two backward() calls run the encoder's backward once per cotangent
    # and add the second result onto the first, one fp32 addition per element: bit for bit the two ops-level
    # calls with `accumulate`.  One call on the summed cotangent rounds elsewhere, so it is not the comparison.
    ep, ids, mask, tape_e = step["encoder_args"]
    d_enc_reg, d_enc_u = step["d_enc_parts"]
    first = ops.encoder_backward(ep, ids, mask, tape_e, d_enc_reg, HEADS)
    mel_only = [g.clone() for g in first]
    both = ops.encoder_backward(ep, ids, mask, tape_e, d_enc_u, HEADS, accumulate=first)
    for p, g, m in zip(model.text_encoder.parameters(), both, mel_only):
        assert torch.equal(p.grad, g) and not torch.equal(g, m)
    model.enable_backward(False).eval()


def test_eval_mode_audio_follows_the_vocoders_own_switch(gpu):
    model, x = _new_model(gpu), _inputs(gpu)
    model.enable_backward()
    assert model.vocoder.backward_enabled is False and not model.training
    kw = dict(target_durations=x["dur"], max_target_length=x["T"])
    out = model(x["ids"], x["lengths"], **kw)
    assert out["audio_output"] is not None and out["audio_output"].grad_fn is None  # the caller's switch is off
    assert out["audio_output"].shape == (B, 1, 64 * x["T"]) and out["mel_output"].grad_fn is not None
    model.vocoder.enable_backward()
    out = model(x["ids"], x["lengths"], **kw)
    audio = out["audio_output"]
    assert audio.grad_fn is not None and audio.shape == (B, 1, 64 * x["T"])
    alone = copy.deepcopy(model.vocoder).enable_backward(False)
    with torch.no_grad():
        assert torch.equal(audio.detach(), alone(out["mel_output"].detach().transpose(1, 2)))
    (audio ** 2).sum().backward()
    for part in (model.vocoder, model.decoder, model.text_encoder):
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
                   for p in part.parameters())
    assert all(p.grad is None for p in model.duration_predictor.parameters())  # target durations: no path to it
    model.vocoder.enable_backward(False)
    model.enable_backward(False)
