"""GPU: the vocoder's training forward and backward (m2_vocoder_train_forward,
m2_vocoder_backward, SimpleVocoder.enable_backward) against torch autograd on
the CPU in float64.  Nothing here reads the reference: the oracle is the
module's own nn layers, deep-copied to the CPU (tests/golden/vocoder_backward_oracle.py).

No bar comes from the GPU's output.  Per tensor g:
    |g_gpu - g_f64| <= 32 x max(s, 2^-24) x max|g_f64|,
s the largest relative deviation, over the tensors of the case, of CPU float32
autograd from float64 autograd, computed here (the bar of
test_gpu_losses_backward.py).

LeakyReLU kinks are accounted exactly.  The float64 oracle applies each
LeakyReLU as a product with a constant slope mask taken from the sign of the
GPU's stored map, read from the tape; wherever that sign differs from the
float64 pre-activation, |pre_f64| must be within the forward bar of the map,
32 x max(s_fwd, 2^-24) x max|map| (s_fwd: CPU float32 against float64 on that
map), and at most 4 elements per case may differ: a cap, not a measurement.
The count is printed.

The three kernels alone are checked at c in {1, 2, 8, 16, 64, 128} and L in
{1, 2, 63, 64, 65, 4480} (one position, shorter than the halo, around a wave
and a tile, several tiles and chunks).  voc_dw_narrow_kernel exists for fewer
than 16 output channels: it runs c in {1, 2, 8} and the ConvTranspose1d forms
(k = 2r, stride r) at every length, and c >= 16 must be refused by it, since
those rows go to the MFMA.

The optimizer step compares float32 parameters after the update with the same
update done in float64: the gradient bar times the learning rate, plus the
rounding of the stored float32 parameter itself, 2^-24 x max|p|.
"""
import copy
import ctypes
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

sys.path.insert(0, str(GOLDEN))
import vocoder_backward_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
KINK_CAP = 4
LR, CLIP = 0.05, 1.0
CHANNELS = (1, 2, 8, 16, 64, 128)
LENGTHS = (1, 2, 63, 64, 65, 4480)


def _rel(a, b):
    return float((a.double() - b).abs().max()) / float(b.abs().max())


def _dims(case):
    return orc.CASES[case][:4]


_EXPECT = {}


def _expect(case, gpu):
    """The case's module on the GPU, its inputs, the ops-level result, and the float64 gradients with the
    GPU's side of every kink; computed once per case and never changed."""
    if case in _EXPECT:
        return _EXPECT[case]
    from m2amd import ops
    M, C, B, T = _dims(case)
    voc = orc.make_vocoder(case)
    mel, dy = orc.make_inputs(case)
    v64, v32 = orc.cpu_copy(voc, torch.float64), orc.cpu_copy(voc, torch.float32)
    g64, m64, _, pre64 = orc.gradients(v64, mel.double(), dy.double())
    g32, m32, _, pre32 = orc.gradients(v32, mel, dy)
    s = max(_rel(a, b) for a, b in zip(g32 + [m32], g64 + [m64]))
    gvoc = copy.deepcopy(voc).to(gpu)
    params = [p.detach() for p in gvoc.parameters()]
    audio, tape = ops.vocoder_train_forward(params, mel.to(gpu))
    maps = ops.vocoder_tape_maps(tape, M, C, B, T)
    positive = {}
    for k in range(4):
        positive[f"u{k}"] = maps[f"a{k}"].cpu() > 0
        positive[f"v{k}"] = maps[f"lv{k}"].cpu() > 0
    grads, d_mel, _, pre = orc.gradients(v64, mel.double(), dy.double(), positive)
    kinks, total = 0, 0
    for name in orc.PRE:
        top = float(pre64[name].abs().max())
        s_fwd = float((pre32[name].double() - pre64[name]).abs().max()) / top
        differ = (pre[name] > 0) != positive[name]
        assert bool((pre[name].abs()[differ] <= 32.0 * max(s_fwd, EPS) * top).all()), \
            (case, name, "a resolvable pre-activation changed sign")
        kinks += int(differ.sum())
        total += differ.numel()
    print(f"{case}: {kinks} of {total} pre-activations take the other LeakyReLU slope on the GPU; s = {s:.3e}")
    assert kinks <= KINK_CAP, case
    got_mel, got = ops.vocoder_backward(params, mel.to(gpu), tape, dy.to(gpu))
    _EXPECT[case] = {"voc": gvoc, "params": params, "mel": mel.to(gpu), "dy": dy.to(gpu), "audio": audio, "tape": tape,
                     "grads": grads, "d_mel": d_mel, "s": s, "got": got, "got_mel": got_mel}
    return _EXPECT[case]


# ---- forward -----------------------------------------------------------------------

@pytest.mark.parametrize("case", list(orc.CASES))
def test_train_forward_is_the_module_forward_bit_for_bit(gpu, case):
    from m2amd import ops
    e = _expect(case, gpu)
    M, C, B, T = _dims(case)
    with torch.no_grad():
        want = e["voc"](e["mel"])
    assert e["voc"].backward_enabled is False and want.grad_fn is None
    assert e["audio"].shape == (B, 1, 64 * T) and torch.equal(e["audio"], want)
    maps = ops.vocoder_tape_maps(e["tape"], M, C, B, T)
    assert list(maps) == ["h", "a0", "lv0", "x1", "a1", "lv1", "x2", "a2", "lv2", "x3", "a3", "lv3", "x4", "y"]
    assert torch.equal(maps["y"], want)
    p = e["params"]
    h = ops.conv1d(e["mel"], p[0], p[1])
    assert torch.equal(maps["h"], h)
    a0 = ops.conv_transpose1d(h, p[2], p[3], 4, act=ops.ACT_LEAKY)
    assert torch.equal(maps["a0"], a0)
    lv0 = ops.conv1d(a0, p[10], p[11], act=ops.ACT_LEAKY)
    assert torch.equal(maps["lv0"], lv0)
    assert torch.equal(maps["x1"], ops.conv1d(lv0, p[12], p[13], residual=a0))
    assert maps["x4"].shape == (B, C // 16, 64 * T)


def test_forward_inside_a_model_is_the_stand_alone_module(gpu):
    from models.tts_model import M2TTSModel
    torch.manual_seed(11)
    model = M2TTSModel().to(gpu).eval()
    mel = torch.randn(2, 64, 9, device=gpu)
    alone = copy.deepcopy(model.vocoder)
    with torch.no_grad():
        want = alone(mel)  # the copy is no one's vocoder: the per-op path
        split = model.vocoder(mel)
    assert model.vocoder.enable_backward() is model.vocoder
    try:
        got = model.vocoder(mel)
        assert got.grad_fn is not None and torch.equal(got.detach(), want)
        with torch.no_grad():
            quiet = model.vocoder(mel)
        assert quiet.grad_fn is None and torch.equal(quiet, split)  # today's path: the split-f16 handle
        out = model(torch.randint(1, 50, (1, 7), device=gpu))  # M2TTSModel.forward carries no graph
        assert out["audio_output"].grad_fn is None and out["mel_output"].grad_fn is None
    finally:
        model.vocoder.enable_backward(False)
    assert model.vocoder(mel).grad_fn is None


# ---- the chain ---------------------------------------------------------------------

@pytest.mark.parametrize("case", list(orc.CASES))
def test_chain_matches_float64_autograd(gpu, case):
    e = _expect(case, gpu)
    bar = 32.0 * max(e["s"], EPS)
    names = list(e["voc"].state_dict()) + ["d_mel"]
    assert len(e["got"]) == 28
    worst = 0.0
    for name, g, ref in zip(names, e["got"] + [e["got_mel"]], e["grads"] + [e["d_mel"]]):
        assert g.shape == ref.shape and g.dtype == torch.float32 and g.is_cuda, (case, name)
        err = _rel(g.cpu(), ref)
        worst = max(worst, err)
        assert err <= bar, (case, name, err, bar)
    print(f"{case}: worst rel max err {worst:.3e}, cpu float32 {e['s']:.3e}, bar {bar:.3e}")


# ---- the three kernels alone -------------------------------------------------------

def _check(what, got, want, single):
    s = max(_rel(a, b) for a, b in zip(single, want))
    bar = 32.0 * max(s, EPS)
    for i, (g, ref) in enumerate(zip(got, want)):
        assert g.shape == ref.shape and g.dtype == torch.float32, (what, i)
        err = _rel(g.cpu(), ref)
        assert err <= bar, (what, i, err, bar)
    return bar


@pytest.mark.parametrize("c", CHANNELS)
def test_output_conv_backward_alone(gpu, c):
    from m2amd import ops
    g = torch.Generator().manual_seed(500 + c)
    for L in LENGTHS:
        x = torch.randn(2, c, L, generator=g)
        w = torch.randn(1, c, 3, generator=g) / (3 * c) ** 0.5
        b = torch.randn(1, generator=g) * 0.05
        gy = torch.randn(2, 1, L, generator=g)

        def autograd(dtype):
            xx, ww, bb = (t.to(dtype).requires_grad_() for t in (x, w, b))
            y = torch.tanh(F.conv1d(xx, ww, bb, padding=1))
            return torch.autograd.grad(y, (xx, ww, bb), gy.to(dtype)), y.detach()

        (want, y64), (single, _) = autograd(torch.float64), autograd(torch.float32)
        got = ops.vocoder_out_backward(gy.to(gpu), y64.float().to(gpu), x.to(gpu), w.to(gpu))
        _check(f"out c {c} L {L}", got, want, single)
        again = ops.vocoder_out_backward(gy.to(gpu), y64.float().to(gpu), x.to(gpu), w.to(gpu))
        assert all(torch.equal(p, q) for p, q in zip(got, again))


@pytest.mark.parametrize("c", CHANNELS)
def test_resblock_backward_alone(gpu, c):
    from m2amd import ops
    g = torch.Generator().manual_seed(600 + c)
    for L in LENGTHS:
        u = torch.randn(2, c, L, generator=g)
        w1, w2 = (torch.randn(c, c, 3, generator=g) / (3 * c) ** 0.5 for _ in range(2))
        b1 = torch.randn(c, generator=g) * 0.05
        g_r = torch.randn(2, c, L, generator=g)
        slope = lambda pos, dtype: torch.where(pos, torch.ones((), dtype=dtype), torch.full((), 0.1, dtype=dtype))  # noqa: E731
        pos_u = u > 0
        pos_v = F.conv1d(u.double() * slope(pos_u, torch.float64), w1.double(), b1.double(), padding=1) > 0

        def autograd(dtype):
            uu = u.to(dtype).requires_grad_()
            a = uu * slope(pos_u, dtype)
            v = F.conv1d(a, w1.to(dtype), b1.to(dtype), padding=1)
            lv = v * slope(pos_v, dtype)
            out = F.conv1d(lv, w2.to(dtype), None, padding=1) + a
            gu, gv = torch.autograd.grad(out, (uu, v), g_r.to(dtype))
            return (gv, gu), a.detach(), lv.detach()

        (want, a64, lv64), (single, _, _) = autograd(torch.float64), autograd(torch.float32)
        a32, lv32 = a64.float(), lv64.float()
        assert bool(((a32 > 0) == pos_u).all()) and bool(((lv32 > 0) == pos_v).all())  # rounding keeps the sign
        args = [t.to(gpu) for t in (g_r, lv32, a32, w1, w2)]
        got = ops.resblock_backward(*args)
        _check(f"resblock c {c} L {L}", got, want, single)
        again = ops.resblock_backward(*args)
        assert all(torch.equal(p, q) for p, q in zip(got, again))


NARROW = [(c, c, 3, 1, 1) for c in (1, 2, 8)] + [(4, 8, 8, 4, 2), (2, 4, 4, 2, 1), (15, 15, 3, 1, 1)]


@pytest.mark.parametrize("cin,cout,k,stride,pad", NARROW)
def test_narrow_weight_gradient_alone(gpu, cin, cout, k, stride, pad):
    from m2amd import ops
    g = torch.Generator().manual_seed(700 + cin * 16 + cout)
    for Lo in LENGTHS:
        L = Lo * stride  # (L + 2 pad - k) // stride + 1 = Lo for both forms
        assert (L + 2 * pad - k) // stride + 1 == Lo
        x = torch.randn(3, cin, L, generator=g)
        dy = torch.randn(3, cout, Lo, generator=g)

        def autograd(dtype):
            w = torch.zeros(cout, cin, k, dtype=dtype, requires_grad=True)
            b = torch.zeros(cout, dtype=dtype, requires_grad=True)
            return torch.autograd.grad(F.conv1d(x.to(dtype), w, b, stride, pad), (w, b), dy.to(dtype))

        got = ops.conv1d_narrow_dw(x.to(gpu), dy.to(gpu), k, stride=stride, padding=pad)
        _check(f"narrow {cin}->{cout} k{k} s{stride} Lo {Lo}", got, autograd(torch.float64), autograd(torch.float32))
        assert all(torch.equal(p, q) for p, q in
                   zip(got, ops.conv1d_narrow_dw(x.to(gpu), dy.to(gpu), k, stride=stride, padding=pad)))


@pytest.mark.parametrize("c", [16, 64, 128])
def test_narrow_kernel_refuses_the_rows_of_the_mfma(gpu, c):
    from m2amd import _lib
    lib = _lib.load()
    x = torch.zeros(1, c, 64, device=gpu)
    out = torch.full((c * c * 3,), -1.0, device=gpu)
    assert lib.m2_conv1d_narrow_dw_workspace_bytes(3, 1, 1, 1, c, c, 64) == 0
    assert lib.m2_conv1d_narrow_dw(x.data_ptr(), x.data_ptr(), 3, 1, 1, 1, c, c, 64, out.data_ptr(), None,
                                   out.data_ptr(), out.numel() * 4, None) == -2
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())  # nothing was launched


# ---- determinism, batching, accumulation -------------------------------------------

@pytest.mark.parametrize("case", ["tiles", "thin"])
def test_determinism_batching_and_accumulation(gpu, case):
    from m2amd import ops
    e = _expect(case, gpu)
    B = _dims(case)[2]
    d_mel, grads = ops.vocoder_backward(e["params"], e["mel"], e["tape"], e["dy"])
    assert torch.equal(d_mel, e["got_mel"]) and all(torch.equal(a, b) for a, b in zip(grads, e["got"]))
    for b in range(B):
        mel_b, dy_b = e["mel"][b:b + 1].contiguous(), e["dy"][b:b + 1].contiguous()
        audio_b, tape_b = ops.vocoder_train_forward(e["params"], mel_b)
        assert torch.equal(audio_b, e["audio"][b:b + 1])
        alone, _ = ops.vocoder_backward(e["params"], mel_b, tape_b, dy_b, need=[False] * 28)
        assert torch.equal(alone[0], d_mel[b]), (case, b)
    onto = [g.clone() for g in grads]
    d_mel2, twice = ops.vocoder_backward(e["params"], e["mel"], e["tape"], e["dy"], out=onto)
    assert torch.equal(d_mel2, d_mel)  # d_mel is overwritten regardless
    assert all(t is o for t, o in zip(twice, onto)) and all(torch.equal(t, 2.0 * g) for t, g in zip(twice, grads))


# ---- ABI ---------------------------------------------------------------------------

def test_abi_conventions(gpu):
    from m2amd import _lib, ops
    lib = _lib.load()
    case = "odd"
    e = _expect(case, gpu)
    M, C, B, T = _dims(case)
    need = [i % 3 != 1 for i in range(28)]
    d_mel, some = ops.vocoder_backward(e["params"], e["mel"], e["tape"], e["dy"], need_mel=False, need=need)
    assert d_mel is None
    for i, (g, full) in enumerate(zip(some, e["got"])):
        assert (g is None) == (not need[i]) and (g is None or torch.equal(g, full)), i
    only_mel, none = ops.vocoder_backward(e["params"], e["mel"], e["tape"], e["dy"], need=[False] * 28)
    assert all(g is None for g in none) and torch.equal(only_mel, e["got_mel"])

    pp = (ctypes.c_void_p * 28)(*[p.data_ptr() for p in e["params"]])
    out = [torch.full_like(p, -1.0) for p in e["params"]]
    gp = (ctypes.c_void_p * 28)(*[g.data_ptr() for g in out])
    audio = torch.full((B, 1, 64 * T), -2.0, device=gpu)
    tape_bytes = lib.m2_vocoder_tape_bytes(M, C, B, T)
    ws_bytes = lib.m2_vocoder_backward_workspace_bytes(M, C, B, T)
    tape = torch.empty(tape_bytes, dtype=torch.uint8, device=gpu)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=gpu)
    mel, dy = e["mel"].data_ptr(), e["dy"].data_ptr()
    fwd = lambda b, t, nbytes: lib.m2_vocoder_train_forward(pp, M, C, mel, b, t, audio.data_ptr(), tape.data_ptr(),  # noqa: E731
                                                            nbytes, None)
    bwd = lambda b, t, nbytes: lib.m2_vocoder_backward(pp, M, C, mel, b, t, e["tape"].data_ptr(), dy, None, gp, 0,  # noqa: E731
                                                       ws.data_ptr(), nbytes, None)
    assert fwd(B, T, tape_bytes - 512) == -1 and b"tape too small" in lib.m2_last_error()
    assert bwd(B, T, ws_bytes - 512) == -1 and b"workspace too small" in lib.m2_last_error()
    assert fwd(0, T, 0) == 0 and fwd(B, 0, 0) == 0 and bwd(0, T, 0) == 0 and bwd(B, 0, 0) == 0
    pp[5] = None
    assert fwd(B, T, tape_bytes) == -1 and bwd(B, T, ws_bytes) == -1
    pp[5] = e["params"][5].data_ptr()
    torch.cuda.synchronize()
    assert bool((audio == -2.0).all()) and all(bool((g == -1.0).all()) for g in out)  # nothing was launched
    assert fwd(B, T, tape_bytes) == 0 and bwd(B, T, ws_bytes) == 0  # the queried sizes are accepted
    torch.cuda.synchronize()
    assert torch.equal(audio, e["audio"]) and all(torch.equal(g, w) for g, w in zip(out, e["got"]))


# ---- the module --------------------------------------------------------------------

def _zero(params):
    for p in params:
        p.grad = None


def test_module_backward(gpu):
    e = _expect("s1", gpu)
    voc = copy.deepcopy(e["voc"])
    params = list(voc.parameters())
    mel, dy = e["mel"], e["dy"]
    assert all(p.requires_grad for p in params) and torch.is_grad_enabled()
    assert voc(mel).grad_fn is None and voc(mel.clone().requires_grad_()).grad_fn is None  # the switch is off
    assert voc.enable_backward() is voc
    with torch.no_grad():
        assert voc(mel).grad_fn is None
    audio = voc(mel)
    assert audio.grad_fn is not None and torch.equal(audio.detach(), e["audio"])
    audio.backward(dy)
    assert mel.grad is None
    assert all(torch.equal(p.grad, g) for p, g in zip(params, e["got"]))
    voc(mel).backward(dy)  # a second backward accumulates
    assert all(torch.equal(p.grad, 2.0 * g) for p, g in zip(params, e["got"]))
    _zero(params)
    x = mel.clone().requires_grad_()
    strided = torch.stack([dy, -dy], dim=-1)[..., 0]  # any [B,1,64T] tensor: made contiguous
    assert not strided.is_contiguous()
    voc(x).backward(strided)
    assert torch.equal(x.grad, e["got_mel"]) and all(torch.equal(p.grad, g) for p, g in zip(params, e["got"]))
    with pytest.raises(RuntimeError):  # once differentiable
        (gw,) = torch.autograd.grad(voc(mel), params[:1], dy, create_graph=True)
        gw.sum().backward()
    # frozen parameters get None
    frozen = [params[2], params[13], params[27]]
    for p in frozen:
        p.requires_grad_(False)
    _zero(params)
    voc(mel).backward(dy)
    assert all(p.grad is None for p in frozen)
    assert all(torch.equal(p.grad, g) for p, g in zip(params, e["got"]) if not any(p is f for f in frozen))
    for p in params:
        p.requires_grad_(False)
    assert voc(mel).grad_fn is None  # nothing requires grad: today's path
    x = mel.clone().requires_grad_()
    voc(x).backward(dy)  # the mel alone
    assert torch.equal(x.grad, e["got_mel"]) and all(p.grad is None for p in frozen)
    for p in params:
        p.requires_grad_(True)
    assert voc.enable_backward(False) is voc and voc(mel).grad_fn is None


def test_generator_step_reaches_the_vocoder(gpu):
    """Stage1 model, B = 2, T = 17: total_loss.backward() leaves in the vocoder's .grad exactly what
    ops.vocoder_backward gives for the audio gradient of a second, identical call."""
    from m2amd import ops
    from models.tts_model import M2TTSModel
    from training.losses import CombinedTTSLoss
    torch.manual_seed(21)
    model = M2TTSModel().to(gpu).eval()
    loss = CombinedTTSLoss().eval().to(gpu).enable_backward(spectral=True)
    model.vocoder.enable_backward()
    params = list(model.vocoder.parameters())
    B, T, M, S = 2, 17, 64, 5
    g = torch.Generator().manual_seed(22)
    mel = torch.randn(B, M, T, generator=g).to(gpu)
    # as in the trainer, every prediction comes from the model: total_loss carries a graph only then
    kw = {"mel_pred": torch.randn(B, T, M, generator=g).to(gpu).requires_grad_(),
          "mel_target": torch.randn(B, M, T, generator=g).to(gpu),
          "duration_pred": (torch.rand(B, S, generator=g) * 4 + 0.5).to(gpu).requires_grad_(),
          "duration_target": (torch.rand(B, S, generator=g) * 4 + 0.5).to(gpu),
          "audio_target": torch.tanh(torch.randn(B, 1, 64 * T, generator=g)).to(gpu), "mel_lengths": None}
    try:
        audio = model.vocoder(mel)
        assert audio.grad_fn is not None and audio.shape == (B, 1, 1088)
        total = loss(audio_pred=audio, **kw)["total_loss"]
        assert total.grad_fn is not None
        total.backward()
        got = [p.grad.clone() for p in params]
        assert all(p.grad is None for p in loss.get_discriminator_parameters())
        audio2 = model.vocoder(mel)
        total2 = loss(audio_pred=audio2, **kw)["total_loss"]
        assert torch.equal(total2.detach(), total.detach()) and torch.equal(audio2.detach(), audio.detach())
        (g_audio,) = torch.autograd.grad(total2, audio2)
        assert g_audio.shape == audio.shape and float(g_audio.abs().max()) > 0
        audio3, tape = ops.vocoder_train_forward(params, mel)
        assert torch.equal(audio3, audio.detach())
        _, want = ops.vocoder_backward(params, mel, tape, g_audio, need_mel=False)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        assert all(float(a.abs().max()) > 0 for a in got)
    finally:
        loss.enable_backward(False)
        model.vocoder.enable_backward(False)


def test_optimizer_step_matches_float64(gpu):
    """zero_grad, backward of sum(audio dy), clip_grad_norm_, SGD step on a model's vocoder, and the next
    module call on the updated weights."""
    from models.tts_model import M2TTSModel
    e = _expect("odd", gpu)
    torch.manual_seed(31)
    model = M2TTSModel().to(gpu).eval()
    model.vocoder.load_state_dict(e["voc"].state_dict())
    model.vocoder.enable_backward()
    params = list(model.vocoder.parameters())
    mel, dy = e["mel"], e["dy"]
    opt = torch.optim.SGD(params, lr=LR)
    opt.zero_grad()
    (model.vocoder(mel) * dy).sum().backward()
    assert all(torch.equal(p.grad, g) for p, g in zip(params, e["got"]))
    torch.nn.utils.clip_grad_norm_(params, CLIP)
    opt.step()

    p64 = [p.detach().cpu().double().requires_grad_() for p in e["params"]]
    for p, g in zip(p64, e["grads"]):
        p.grad = g.clone()
    norm = torch.nn.utils.clip_grad_norm_(p64, CLIP)
    assert float(norm) > CLIP  # the clipping acts
    torch.optim.SGD(p64, lr=LR).step()
    bar_g = 32.0 * max(e["s"], EPS)
    for i, (p, q, g) in enumerate(zip(params, p64, e["grads"])):
        err = float((p.detach().cpu().double() - q.detach()).abs().max())
        bar = LR * bar_g * float(g.abs().max()) + EPS * float(q.detach().abs().max())
        assert err <= bar, (i, err, bar)
        assert not torch.equal(p.detach(), e["params"][i])  # every parameter moved
    after = model.vocoder(mel)
    alone = copy.deepcopy(model.vocoder).enable_backward(False)
    with torch.no_grad():
        want = alone(mel)
    assert after.grad_fn is not None and torch.equal(after.detach(), want)  # no stale pack is read
    assert not torch.equal(want, e["audio"])
