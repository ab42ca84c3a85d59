"""GPU: the mel decoder's training forward and backward (m2_decoder_train_forward,
m2_decoder_backward, MelDecoder.enable_backward) against torch autograd on the
CPU in float64.  Nothing here reads the reference: the oracle is the module's
own nn layers, deep-copied to the CPU (tests/golden/decoder_backward_oracle.py).

No bar comes from the GPU's output.  Per tensor g:
    |g_gpu - g_f64| <= 32 x max(s, 2^-24) x max|g_f64|,
s the largest relative deviation, over the tensors of the case, of CPU float32
autograd from float64 autograd, computed here (the bar of
test_gpu_vocoder_backward.py).

ReLU kinks are accounted exactly.  The float64 oracle applies each ReLU as a
product with a constant 0/1 mask taken from the GPU's stored map (h > 0), read
from the tape; wherever that predicate differs from the float64
pre-activation's sign, |pre_f64| must be within the forward bar of the map,
32 x max(s_fwd, 2^-24) x max|map| (s_fwd: CPU float32 against float64 on that
map), and at most 4 elements per case may differ: a cap, not a measurement.
The count is printed.

The kernels alone: the attention's backward at head_dim in {16, 32, 48, 64} and
N in {1, 2, 63, 64, 65, 129, 511}, unmasked and with lengths (N, max(1, N//2),
0), where the fully masked utterance's dQ and dK must be exactly 0; the linear
data gradient with each epilogue and the weight gradient with and without the
re-formed LayerNorm at (K, N) in {(64,192), (96,288), (128,384), (128,64),
(64,5), (96,80)} and R in {1, 63, 64, 65, 260}, the weight gradient at R = 4480
too, where several splits run.

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
import decoder_backward_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
KINK_CAP = 4
LR = 0.05
HEAD_DIMS = (16, 32, 48, 64)
LENGTHS = (1, 2, 63, 64, 65, 129, 511)
SHAPES = ((64, 192), (96, 288), (128, 384), (128, 64), (64, 5), (96, 80))
ROWS = (1, 63, 64, 65, 260)


def _rel(a, b):
    return float((a.double() - b).abs().max()) / float(b.abs().max())


def _dims(case):
    return orc.CASES[case]


_EXPECT = {}


def _expect(case, gpu):
    """The case's module on the GPU, its inputs, the ops-level result, and the float64 gradients with the
    GPU's side of every kink; computed once per case and never changed."""
    if case in _EXPECT:
        return _EXPECT[case]
    from m2amd import ops
    H, M, layers, heads, B, T = _dims(case)
    dec = orc.make_decoder(case)
    x, dy = orc.make_inputs(case)
    d64, d32 = orc.cpu_copy(dec, torch.float64), orc.cpu_copy(dec, torch.float32)
    g64, x64, _, pre64 = orc.gradients(d64, x.double(), dy.double())
    g32, x32, _, pre32 = orc.gradients(d32, x, dy)
    s = max(_rel(a, b) for a, b in zip(g32 + [x32], g64 + [x64]))
    gdec = copy.deepcopy(dec).to(gpu)
    params = [p.detach() for p in gdec.parameters()]
    mel, tape = ops.decoder_train_forward(params, x.to(gpu), heads)
    maps = ops.decoder_tape_maps(tape, H, M, layers, heads, B, T)
    positive = [m["h"].cpu() > 0 for m in maps]
    grads, d_x, _, pre = orc.gradients(d64, x.double(), dy.double(), positive)
    kinks, total = 0, 0
    for l in range(layers):
        top = float(pre64[l].abs().max())
        s_fwd = float((pre32[l].double() - pre64[l]).abs().max()) / top
        differ = (pre[l] > 0) != positive[l]
        assert bool((pre[l].abs()[differ] <= 32.0 * max(s_fwd, EPS) * top).all()), \
            (case, l, "a resolvable pre-activation changed sign")
        kinks += int(differ.sum())
        total += differ.numel()
    print(f"{case}: {kinks} of {total} pre-activations take the other ReLU side on the GPU; s = {s:.3e}")
    assert kinks <= KINK_CAP, case
    got_x, got = ops.decoder_backward(params, x.to(gpu), tape, dy.to(gpu), heads)
    _EXPECT[case] = {"dec": gdec, "params": params, "x": x.to(gpu), "dy": dy.to(gpu), "mel": mel, "tape": tape,
                     "grads": grads, "d_x": d_x, "s": s, "got": got, "got_x": got_x}
    return _EXPECT[case]


# ---- forward -----------------------------------------------------------------------

@pytest.mark.parametrize("case", list(orc.CASES))
def test_train_forward_is_the_module_forward_bit_for_bit(gpu, case):
    from m2amd import ops
    e = _expect(case, gpu)
    H, M, layers, heads, B, T = _dims(case)
    with torch.no_grad():
        want = e["dec"](e["x"])
    assert e["dec"].backward_enabled is False and want.grad_fn is None
    assert e["mel"].shape == (B, T, M) and torch.equal(e["mel"], want)
    on = copy.deepcopy(e["dec"]).enable_backward()
    got = on(e["x"])  # the parameters require grad
    assert got.grad_fn is not None and torch.equal(got.detach(), want)
    maps = ops.decoder_tape_maps(e["tape"], H, M, layers, heads, B, T)
    assert len(maps) == layers and list(maps[0]) == ["qkv", "att", "x_mid", "h", "x_out"]
    p = e["params"]
    qkv = ops.linear(e["x"], p[0], ln=(p[7], p[8]))
    assert torch.equal(maps[0]["qkv"], qkv)
    att = ops.attention_core(qkv, heads, None)
    assert torch.equal(maps[0]["att"], att)
    x_mid = ops.linear(att, p[1], p[2], residual=e["x"])
    assert torch.equal(maps[0]["x_mid"], x_mid)
    h = ops.linear(x_mid, p[3], p[4], ln=(p[9], p[10]), act=ops.ACT_RELU)
    assert torch.equal(maps[0]["h"], h) and float(h.min()) == 0.0
    assert torch.equal(maps[0]["x_out"], ops.linear(h, p[5], p[6], residual=x_mid))
    assert maps[-1]["h"].shape == (B, T, 2 * H)


def test_forward_inside_a_model_is_the_stand_alone_module(gpu):
    from models.tts_model import M2TTSModel
    torch.manual_seed(11)
    model = M2TTSModel().to(gpu).eval()
    x = torch.randn(2, 9, 64, device=gpu)
    alone = copy.deepcopy(model.decoder)
    with torch.no_grad():
        want = alone(x)  # the copy is no one's decoder: the per-op path
        fused = model.decoder(x)
    assert model.decoder.enable_backward() is model.decoder
    try:
        got = model.decoder(x)
        assert got.grad_fn is not None and torch.equal(got.detach(), want)
        with torch.no_grad():
            quiet = model.decoder(x)
        assert quiet.grad_fn is None and torch.equal(quiet, fused)  # today's path: the handle's fused layers
        out = model(torch.randint(1, 50, (1, 7), device=gpu))  # M2TTSModel.forward carries no graph
        assert out["mel_output"].grad_fn is None
    finally:
        model.decoder.enable_backward(False)
    assert model.decoder(x).grad_fn is None


# ---- the chain ---------------------------------------------------------------------

@pytest.mark.parametrize("case", list(orc.CASES))
def test_chain_matches_float64_autograd(gpu, case):
    e = _expect(case, gpu)
    layers = _dims(case)[2]
    bar = 32.0 * max(e["s"], EPS)
    names = list(e["dec"].state_dict()) + ["d_x"]
    assert len(e["got"]) == 11 * layers + 4
    worst = 0.0
    for name, g, ref in zip(names, e["got"] + [e["got_x"]], e["grads"] + [e["d_x"]]):
        assert g.shape == ref.shape and g.dtype == torch.float32 and g.is_cuda, (case, name)
        err = _rel(g.cpu(), ref)
        worst = max(worst, err)
        assert err <= bar, (case, name, err, bar)
    print(f"{case}: worst rel max err {worst:.3e}, cpu float32 {e['s']:.3e}, bar {bar:.3e}")


# ---- the kernels alone -------------------------------------------------------------

def _check(what, got, want, single):
    s = max(_rel(a, b) for a, b in zip(single, want) if float(b.abs().max()) > 0)
    bar = 32.0 * max(s, EPS)
    for i, (g, ref) in enumerate(zip(got, want)):
        assert g.shape == ref.shape and g.dtype == torch.float32, (what, i)
        top = float(ref.abs().max())
        err = float((g.cpu().double() - ref).abs().max())
        assert err <= bar * top, (what, i, err, bar * top)
    return bar


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_attention_backward_alone(gpu, hd):
    from m2amd import ops
    heads, B = 2, 3
    H = heads * hd
    g = torch.Generator().manual_seed(800 + hd)
    for N in LENGTHS:
        qkv = torch.randn(B, N, 3 * H, generator=g)
        d_att = torch.randn(B, N, H, generator=g)
        lengths = torch.tensor([N, max(1, N // 2), 0])
        mask = torch.arange(N)[None, :] < lengths[:, None]
        for m in (None, mask):
            def autograd(dtype):
                leaf = qkv.to(dtype).requires_grad_()
                att = orc.attention(leaf, heads, m)
                return torch.autograd.grad(att, leaf, d_att.to(dtype)), att.detach()

            (want, att64), (single, _) = autograd(torch.float64), autograd(torch.float32)
            args = (qkv.to(gpu), None if m is None else m.to(gpu), att64.float().to(gpu), d_att.to(gpu), heads)
            got = ops.attention_backward(*args)
            # d_qkv is one tensor: with a single live key dQ and dK vanish by cancellation (softmax of one
            # score is constant), and what is left of them is rounding at the scale of dP, not of themselves
            _check(f"attention hd {hd} N {N} mask {m is not None}", [got], want, single)
            assert torch.equal(got, ops.attention_backward(*args))
            if m is not None:  # the fully masked utterance
                assert float(got[2, :, :2 * H].abs().max()) == 0.0 and float(got[2, :, 2 * H:].abs().max()) > 0


@pytest.mark.parametrize("K,N", SHAPES)
def test_linear_data_gradient_alone(gpu, K, N):
    from m2amd import ops
    g = torch.Generator().manual_seed(900 + K + N)
    for R in ROWS:
        w = torch.randn(N, K, generator=g) / K ** 0.5
        g_y = torch.randn(R, N, generator=g)
        x = torch.randn(R, K, generator=g)
        gamma, beta = torch.randn(K, generator=g) * 0.2 + 1, torch.randn(K, generator=g) * 0.2
        g_res = torch.randn(R, K, generator=g)
        pos = torch.rand(R, K, generator=g) > 0.5
        h = torch.where(pos, torch.rand(R, K, generator=g) + 0.1, torch.zeros(()))

        def plain(dtype, relu):
            leaf = x.to(dtype).requires_grad_()
            y = (leaf * pos.to(dtype) if relu else leaf) @ w.to(dtype).t()
            return torch.autograd.grad(y, leaf, g_y.to(dtype))

        def normed(dtype, res):
            leaf, ga, be = (t.to(dtype).requires_grad_() for t in (x, gamma, beta))
            y = F.layer_norm(leaf, (K,), ga, be, 1e-5) @ w.to(dtype).t()
            outs, cots = ([y, leaf], [g_y.to(dtype), g_res.to(dtype)]) if res else ([y], [g_y.to(dtype)])
            return torch.autograd.grad(outs, (leaf, ga, be), cots)

        dev = lambda *ts: [t.to(gpu) for t in ts]  # noqa: E731
        what = f"K {K} N {N} R {R}"
        for relu in (False, True):
            got = ops.linear_backward_input(*dev(g_y, w), relu_of=h.to(gpu) if relu else None)
            _check(f"dx relu {relu} {what}", [got], plain(torch.float64, relu), plain(torch.float32, relu))
            if relu:
                assert bool((got.cpu()[~pos] == 0).all())
        for res in (False, True):
            kw = dict(ln_x=x.to(gpu), gamma=gamma.to(gpu), g_res=g_res.to(gpu) if res else None)
            got = ops.linear_backward_input(*dev(g_y, w), **kw)
            _check(f"dx ln res {res} {what}", got, normed(torch.float64, res), normed(torch.float32, res))
            assert all(torch.equal(a, b) for a, b in zip(got, ops.linear_backward_input(*dev(g_y, w), **kw)))


@pytest.mark.parametrize("K,N", SHAPES)
def test_linear_weight_gradient_alone(gpu, K, N):
    from m2amd import ops
    g = torch.Generator().manual_seed(950 + K + N)
    for R in ROWS + (4480,):
        g_y = torch.randn(R, N, generator=g)
        x = torch.randn(R, K, generator=g)
        gamma, beta = torch.randn(K, generator=g) * 0.2 + 1, torch.randn(K, generator=g) * 0.2
        for ln in (False, True):
            def autograd(dtype):
                w = torch.zeros(N, K, dtype=dtype, requires_grad=True)
                b = torch.zeros(N, dtype=dtype, requires_grad=True)
                xin = x.to(dtype)
                if ln:
                    xin = F.layer_norm(xin, (K,), gamma.to(dtype), beta.to(dtype), 1e-5)
                return torch.autograd.grad(xin @ w.t() + b, (w, b), g_y.to(dtype))

            kw = dict(ln=(gamma.to(gpu), beta.to(gpu)) if ln else None)
            got = ops.linear_backward_weight(g_y.to(gpu), x.to(gpu), **kw)
            _check(f"dw ln {ln} K {K} N {N} R {R}", got, autograd(torch.float64), autograd(torch.float32))
            assert all(torch.equal(a, b) for a, b in zip(got, ops.linear_backward_weight(g_y.to(gpu), x.to(gpu), **kw)))


# ---- determinism, batching, accumulation -------------------------------------------

@pytest.mark.parametrize("case", ["tiles", "thin", "heads4"])
def test_determinism_batching_and_accumulation(gpu, case):
    from m2amd import ops
    e = _expect(case, gpu)
    layers, heads, B = _dims(case)[2:5]
    n = 11 * layers + 4
    d_x, grads = ops.decoder_backward(e["params"], e["x"], e["tape"], e["dy"], heads)
    assert torch.equal(d_x, e["got_x"]) and all(torch.equal(a, b) for a, b in zip(grads, e["got"]))
    for b in range(B):
        x_b, dy_b = e["x"][b:b + 1].contiguous(), e["dy"][b:b + 1].contiguous()
        mel_b, tape_b = ops.decoder_train_forward(e["params"], x_b, heads)
        assert torch.equal(mel_b, e["mel"][b:b + 1])
        alone, _ = ops.decoder_backward(e["params"], x_b, tape_b, dy_b, heads, need=[False] * n)
        assert torch.equal(alone[0], d_x[b]), (case, b)
    onto = [g.clone() for g in grads]
    d_x2, twice = ops.decoder_backward(e["params"], e["x"], e["tape"], e["dy"], heads, accumulate=onto)
    assert torch.equal(d_x2, d_x)  # d_x is overwritten regardless
    assert all(t is o for t, o in zip(twice, onto)) and all(torch.equal(t, 2.0 * g) for t, g in zip(twice, grads))


# ---- ABI ---------------------------------------------------------------------------

def test_abi_conventions(gpu):
    from m2amd import _lib, ops
    lib = _lib.load()
    case = "odd"
    e = _expect(case, gpu)
    H, M, layers, heads, B, T = dims = _dims(case)
    d4 = dims[:4]
    n = 11 * layers + 4
    need = [i % 3 != 1 for i in range(n)]
    d_x, some = ops.decoder_backward(e["params"], e["x"], e["tape"], e["dy"], heads, need_x=False, need=need)
    assert d_x is None
    for i, (g, full) in enumerate(zip(some, e["got"])):
        assert (g is None) == (not need[i]) and (g is None or torch.equal(g, full)), i
    only_x, none = ops.decoder_backward(e["params"], e["x"], e["tape"], e["dy"], heads, need=[False] * n)
    assert all(g is None for g in none) and torch.equal(only_x, e["got_x"])

    pp = (ctypes.c_void_p * n)(*[p.data_ptr() for p in e["params"]])
    out = [torch.full_like(p, -1.0) for p in e["params"]]
    gp = (ctypes.c_void_p * n)(*[g.data_ptr() for g in out])
    mel = torch.full((B, T, M), -2.0, device=gpu)
    tape_bytes = lib.m2_decoder_tape_bytes(*dims)
    ws_bytes = lib.m2_decoder_backward_workspace_bytes(*dims)
    tape = torch.empty(tape_bytes, dtype=torch.uint8, device=gpu)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=gpu)
    x, dy = e["x"].data_ptr(), e["dy"].data_ptr()
    fwd = lambda b, t, nbytes: lib.m2_decoder_train_forward(pp, *d4, x, b, t, mel.data_ptr(), tape.data_ptr(),  # noqa: E731
                                                            nbytes, None)
    bwd = lambda b, t, nbytes: lib.m2_decoder_backward(pp, *d4, x, b, t, e["tape"].data_ptr(), dy, None, gp, 0,  # noqa: E731
                                                       ws.data_ptr(), nbytes, None)
    assert fwd(B, T, tape_bytes - 512) == -1 and b"tape too small" in lib.m2_last_error()
    assert bwd(B, T, ws_bytes - 512) == -1 and b"workspace too small" in lib.m2_last_error()
    assert fwd(0, T, 0) == 0 and fwd(B, 0, 0) == 0 and bwd(0, T, 0) == 0 and bwd(B, 0, 0) == 0
    pp[5] = None
    assert fwd(B, T, tape_bytes) == -1 and bwd(B, T, ws_bytes) == -1
    pp[5] = e["params"][5].data_ptr()
    torch.cuda.synchronize()
    assert bool((mel == -2.0).all()) and all(bool((g == -1.0).all()) for g in out)  # nothing was launched
    assert fwd(B, T, tape_bytes) == 0 and bwd(B, T, ws_bytes) == 0  # the queried sizes are accepted
    torch.cuda.synchronize()
    assert torch.equal(mel, e["mel"]) and all(torch.equal(g, w) for g, w in zip(out, e["got"]))


# ---- the module --------------------------------------------------------------------

def _zero(params):
    for p in params:
        p.grad = None


def test_module_backward(gpu):
    e = _expect("s1", gpu)
    dec = copy.deepcopy(e["dec"])
    params = list(dec.parameters())
    x, dy = e["x"], e["dy"]
    assert all(p.requires_grad for p in params) and torch.is_grad_enabled()
    assert dec(x).grad_fn is None and dec(x.clone().requires_grad_()).grad_fn is None  # the switch is off
    assert dec.enable_backward() is dec
    with torch.no_grad():
        assert dec(x).grad_fn is None
    mel = dec(x)
    assert mel.grad_fn is not None and torch.equal(mel.detach(), e["mel"])
    mel.backward(dy)
    assert x.grad is None
    assert all(torch.equal(p.grad, g) for p, g in zip(params, e["got"]))
    dec(x).backward(dy)  # a second backward accumulates
    assert all(torch.equal(p.grad, 2.0 * g) for p, g in zip(params, e["got"]))
    _zero(params)
    leaf = x.clone().requires_grad_()
    strided = torch.stack([dy, -dy], dim=-1)[..., 0]  # any [B,T,M] tensor: made contiguous
    assert not strided.is_contiguous()
    dec(leaf).backward(strided)
    assert torch.equal(leaf.grad, e["got_x"]) and all(torch.equal(p.grad, g) for p, g in zip(params, e["got"]))
    with pytest.raises(RuntimeError):  # once differentiable
        (gw,) = torch.autograd.grad(dec(x), params[:1], dy, create_graph=True)
        gw.sum().backward()
    # frozen parameters get None
    frozen = [params[0], params[8], params[13], params[25]]
    for p in frozen:
        p.requires_grad_(False)
    _zero(params)
    dec(x).backward(dy)
    assert all(p.grad is None for p in frozen)
    assert all(torch.equal(p.grad, g) for p, g in zip(params, e["got"]) if not any(p is f for f in frozen))
    for p in params:
        p.requires_grad_(False)
    assert dec(x).grad_fn is None  # nothing requires grad: today's path
    leaf = x.clone().requires_grad_()
    dec(leaf).backward(dy)  # x alone
    assert torch.equal(leaf.grad, e["got_x"]) and all(p.grad is None for p in frozen)
    for p in params:
        p.requires_grad_(True)
    assert dec.enable_backward(False) is dec and dec(x).grad_fn is None


def test_unsupported_shapes_raise(gpu):
    from m2amd import ops
    from models.tts_model import MelDecoder
    for bad in (dict(hidden_dim=160, num_heads=4), dict(hidden_dim=64, num_heads=8), dict(hidden_dim=40, num_heads=1)):
        dec = MelDecoder(**bad).to(gpu)
        with pytest.raises(NotImplementedError):
            dec.enable_backward()
        assert dec.backward_enabled is False
        h = bad["hidden_dim"]
        with pytest.raises(ops.M2Error):
            ops.decoder_train_forward(list(dec.parameters()), torch.zeros(1, 3, h, device=gpu), bad["num_heads"])


def test_generator_step_reaches_the_decoder(gpu):
    """Stage1 model, B = 2, T = 17: the mel comes from MelDecoder(x) with both switches on; after
    total_loss.backward() every decoder parameter has a finite non-zero .grad, the mel's cotangent is the mel
    loss's gradient plus the vocoder's d_mel, and the decoder's d_x is the float64 chain's within the bar."""
    from m2amd import ops
    from models.tts_model import M2TTSModel
    from training.losses import CombinedTTSLoss
    torch.manual_seed(21)
    model = M2TTSModel().to(gpu).eval()
    loss = CombinedTTSLoss().eval().to(gpu).enable_backward(spectral=True)
    model.vocoder.enable_backward()
    model.decoder.enable_backward()
    params = list(model.decoder.parameters())
    heads = 2
    B, T, M, S, H = 2, 17, 64, 5, 64
    g = torch.Generator().manual_seed(22)
    x = torch.randn(B, T, H, generator=g).to(gpu).requires_grad_()
    kw = {"mel_target": torch.randn(B, M, T, generator=g).to(gpu),
          "duration_pred": (torch.rand(B, S, generator=g) * 4 + 0.5).to(gpu).requires_grad_(),
          "duration_target": (torch.rand(B, S, generator=g) * 4 + 0.5).to(gpu),
          "audio_target": torch.tanh(torch.randn(B, 1, 64 * T, generator=g)).to(gpu), "mel_lengths": None}
    try:
        mel = model.decoder(x)  # [B, T, M]
        assert mel.grad_fn is not None and mel.shape == (B, T, M)
        mel.retain_grad()
        audio = model.vocoder(mel.transpose(1, 2))
        assert audio.grad_fn is not None and audio.shape == (B, 1, 64 * T)
        total = loss(mel_pred=mel, audio_pred=audio, **kw)["total_loss"]
        total.backward()
        got = [p.grad.clone() for p in params]
        assert all(bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0 for a in got)
        assert all(p.grad is not None for p in model.vocoder.parameters())
        # the mel's cotangent: the mel loss's own gradient plus the vocoder's d_mel
        # (total_loss carries a graph only when every term has a gradient, so the two parts are taken from a
        # call whose mel_pred and whose vocoder input are separate leaves)
        leaf, other = (mel.detach().clone().requires_grad_() for _ in range(2))
        audio2 = model.vocoder(leaf.transpose(1, 2))
        out2 = loss(mel_pred=other, audio_pred=audio2, **kw)
        assert torch.equal(out2["total_loss"].detach(), total.detach())
        (g_voc,) = torch.autograd.grad(out2["total_loss"], leaf, retain_graph=True)
        (g_loss,) = torch.autograd.grad(out2["mel_loss"], other)
        g_loss = loss.mel_loss_weight * g_loss
        g_mel = mel.grad
        assert float(g_loss.abs().max()) > 0 and float(g_voc.abs().max()) > 0
        top = float(g_mel.abs().max())
        assert float((g_mel - (g_loss + g_voc)).abs().max()) <= 4 * EPS * top  # one fp32 addition of two terms
        # the decoder's own part of the chain against float64, from that cotangent
        mel3, tape = ops.decoder_train_forward(params, x, heads)
        assert torch.equal(mel3, mel.detach())
        want_x, want = ops.decoder_backward(params, x, tape, g_mel, heads)
        assert torch.equal(x.grad, want_x) and all(torch.equal(a, b) for a, b in zip(got, want))
        maps = ops.decoder_tape_maps(tape, H, M, 2, heads, B, T)
        positive = [m["h"].cpu() > 0 for m in maps]
        d64, d32 = orc.cpu_copy(model.decoder, torch.float64), orc.cpu_copy(model.decoder, torch.float32)
        xc, gc = x.detach().cpu(), g_mel.cpu()
        g64, x64, _, _ = orc.gradients(d64, xc.double(), gc.double(), positive)
        g32, x32, _, _ = orc.gradients(d32, xc, gc, positive)
        s = max(_rel(a, b) for a, b in zip(g32 + [x32], g64 + [x64]) if float(b.abs().max()) > 0)
        bar = 32.0 * max(s, EPS)
        assert _rel(x.grad.cpu(), x64) <= bar, (_rel(x.grad.cpu(), x64), bar)
    finally:
        loss.enable_backward(False)
        model.vocoder.enable_backward(False)
        model.decoder.enable_backward(False)


def test_optimizer_step_matches_float64(gpu):
    """zero_grad, backward of sum(mel dy), SGD step on a model's decoder, and the next module call on the
    updated weights."""
    from models.tts_model import M2TTSModel
    e = _expect("s1", gpu)
    torch.manual_seed(31)
    model = M2TTSModel().to(gpu).eval()
    model.decoder.load_state_dict(e["dec"].state_dict())
    model.decoder.enable_backward()
    params = list(model.decoder.parameters())
    x, dy = e["x"], e["dy"]
    opt = torch.optim.SGD(params, lr=LR)
    opt.zero_grad()
    (model.decoder(x) * dy).sum().backward()
    assert all(torch.equal(p.grad, g) for p, g in zip(params, e["got"]))
    opt.step()

    p64 = [p.detach().cpu().double().requires_grad_() for p in e["params"]]
    for p, g in zip(p64, e["grads"]):
        p.grad = g.clone()
    torch.optim.SGD(p64, lr=LR).step()
    bar_g = 32.0 * max(e["s"], EPS)
    for i, (p, q, g) in enumerate(zip(params, p64, e["grads"])):
        err = float((p.detach().cpu().double() - q.detach()).abs().max())
        bar = LR * bar_g * float(g.abs().max()) + EPS * float(q.detach().abs().max())
        assert err <= bar, (i, err, bar)
        assert not torch.equal(p.detach(), e["params"][i])  # every parameter moved
    after = model.decoder(x)
    alone = copy.deepcopy(model.decoder).enable_backward(False)
    with torch.no_grad():
        want = alone(x)
    assert after.grad_fn is not None and torch.equal(after.detach(), want)  # no stale pack is read
    assert not torch.equal(want, e["mel"])
    model.decoder.enable_backward(False)
