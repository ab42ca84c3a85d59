"""GPU: the duration predictor's training forward and backward
(m2_duration_train_forward, m2_duration_backward,
DurationPredictor.enable_backward) against torch autograd on the CPU in
float64.  Nothing here reads the reference: the oracle is the module's own nn
layers, deep-copied to the CPU (tests/golden/duration_backward_oracle.py).

The bar is test_gpu_encoder_backward.py's; no number comes from the GPU's
output.  Per tensor g:
    |g_gpu - g_f64| <= 32 x max(s, 2^-24) x max|g_f64|,
s the largest relative deviation, over the tensors of the case, of CPU float32
autograd from float64 autograd, computed here and printed.

ReLU kinks are accounted as there.  The float64 oracle applies each ReLU as a
product with a constant 0/1 mask taken from the GPU's stored map (y > 0), read
from the tape; wherever that predicate differs from the float64
pre-activation's sign, |pre_f64| must be within the forward bar of the map,
32 x max(s_fwd, 2^-24) x max|map|, and at most 4 elements per case may differ:
a cap, not a measurement.  The count is printed.

The optimizer step compares float32 parameters after the update with the same
update done in float64: the gradient bar times the learning rate, plus the
rounding of the stored float32 parameter itself, 2^-24 x max|p|.
"""
import copy
import ctypes
import sys
import warnings

import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, str(GOLDEN))
import duration_backward_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
KINK_CAP = 4
LR = 0.05


def _rel(a, b):
    return float((a.double() - b).abs().max()) / float(b.abs().max())


def _kinks(what, pre, pre32, pre64, positive):
    """The GPU's side of every kink against the float64 pre-activations: a differing predicate lies within
    the forward bar of its map; returns how many differ."""
    kinks = 0
    for l in range(len(pre)):
        top = float(pre64[l].abs().max())
        s_fwd = float((pre32[l].double() - pre64[l]).abs().max()) / top
        differ = (pre[l] > 0) != positive[l]
        assert bool((pre[l].abs()[differ] <= 32.0 * max(s_fwd, EPS) * top).all()), \
            (what, l, "a resolvable pre-activation changed sign")
        kinks += int(differ.sum())
    return kinks


def _bn_stats(pred):
    from m2amd import ops
    return torch.cat([ops.batchnorm_eval_stats(b.norm.weight, b.norm.bias, b.norm.running_mean, b.norm.running_var,
                                               b.norm.eps) for b in pred.predictor.conv_layers])


_EXPECT = {}


def _expect(case, gpu):
    """The case's module on the GPU, its inputs, the ops-level result, and the float64 gradients with the
    GPU's side of every kink; computed once per case and never changed."""
    if case in _EXPECT:
        return _EXPECT[case]
    from m2amd import ops
    H, B, S, _ = orc.CASES[case]
    pred = orc.make_predictor(case)
    enc, dd = orc.make_inputs(case)
    p64, p32 = orc.cpu_copy(pred, torch.float64), orc.cpu_copy(pred, torch.float32)
    g64, de64, _, pre64 = orc.gradients(p64, enc.double(), dd.double())
    g32, de32, _, pre32 = orc.gradients(p32, enc, dd)
    s = max(_rel(a, b) for a, b in zip(g32 + [de32], g64 + [de64]))
    gpred = copy.deepcopy(pred).to(gpu)
    params = [p.detach() for p in gpred.parameters()]
    bn = _bn_stats(gpred)
    dur, tape = ops.duration_train_forward(params, bn, enc.to(gpu))
    maps = ops.duration_tape_maps(tape, H, B, S)
    positive = [maps["y1"].cpu() > 0, maps["y2"].cpu() > 0]
    grads, d_enc, _, pre = orc.gradients(p64, enc.double(), dd.double(), positive)
    kinks = _kinks(case, pre, pre32, pre64, positive)
    print(f"{case}: {kinks} of {sum(p.numel() for p in pre)} pre-activations take the other ReLU side on the GPU; "
          f"s = {s:.3e}")
    assert kinks <= KINK_CAP, case
    got_enc, got = ops.duration_backward(params, bn, enc.to(gpu), tape, dd.to(gpu))
    _EXPECT[case] = {"pred": gpred, "p64": p64, "p32": p32, "params": params, "bn": bn, "enc": enc.to(gpu),
                     "dd": dd.to(gpu), "dur": dur, "tape": tape, "maps": maps, "positive": positive, "grads": grads,
                     "d_enc": d_enc, "s": s, "got": got, "got_enc": got_enc}
    return _EXPECT[case]


# ---- forward -----------------------------------------------------------------------

@pytest.mark.parametrize("case", list(orc.CASES))
def test_train_forward_is_the_module_forward_bit_for_bit(gpu, case):
    from m2amd import ops
    e = _expect(case, gpu)
    H, B, S, mods = orc.CASES[case]
    with torch.no_grad():
        want = e["pred"](e["enc"])
    assert e["pred"].backward_enabled is False and want.grad_fn is None
    assert e["dur"].shape == (B, S) and torch.equal(e["dur"], want)
    on = copy.deepcopy(e["pred"]).enable_backward()
    got = on(e["enc"])  # the parameters require grad
    assert got.grad_fn is not None and torch.equal(got.detach(), want)
    # the taped maps are the per-op calls
    p, bn = e["params"], e["bn"]
    assert list(e["maps"]) == ["y1", "y2"] and e["maps"]["y1"].shape == (B, H, S)
    x = e["enc"].transpose(1, 2).contiguous()
    y1 = ops.conv1d(x, p[0], p[1], affine=(bn[0], bn[1]), act=ops.ACT_RELU)
    assert torch.equal(e["maps"]["y1"], y1) and float(y1.min()) == 0.0
    y2 = ops.conv1d(y1, p[4], p[5], affine=(bn[4], bn[5]), act=ops.ACT_RELU)
    assert torch.equal(e["maps"]["y2"], y2)
    assert torch.equal(e["dur"], ops.conv1d(y2, p[8], p[9], act=ops.ACT_SOFTPLUS, padding=0).squeeze(1))
    # alpha and beta' are the module's own affine, bit for bit
    n = e["pred"].predictor.conv_layers[1].norm
    alpha, beta = ops.batchnorm_eval_affine(n.weight, n.bias, n.running_mean, n.running_var, n.eps)
    assert torch.equal(bn[4], alpha) and torch.equal(bn[5], beta) and torch.equal(bn[6], n.running_mean)
    if "extreme" in mods:
        z = ops.conv1d(y2, p[8], p[9], padding=0).squeeze(1)
        assert int((z > 20).sum()) > 0 and int((z < -30).sum()) > 0
        assert torch.equal(e["dur"][z > 20], z[z > 20]) and bool((e["dur"] >= 0).all())


def test_forward_inside_a_model_is_the_stand_alone_module(gpu):
    from models.tts_model import M2TTSModel
    torch.manual_seed(12)
    model = M2TTSModel().to(gpu).eval()
    orc.randomize_norms(model.duration_predictor, 12)
    enc = torch.randn(2, 9, 64, generator=torch.Generator().manual_seed(13)).to(gpu)
    alone = copy.deepcopy(model.duration_predictor)
    with torch.no_grad():
        want = alone(enc)  # the copy is no one's predictor: the per-op path
        fused = model.duration_predictor(enc)
    assert model.duration_predictor.enable_backward() is model.duration_predictor
    try:
        got = model.duration_predictor(enc)
        assert got.grad_fn is not None and torch.equal(got.detach(), want)
        with torch.no_grad():
            quiet = model.duration_predictor(enc)
        assert quiet.grad_fn is None and torch.equal(quiet, fused)  # today's path: the handle
        out = model(torch.randint(0, 256, (1, 7), device=gpu))  # the model's own switch is off
        assert out["duration_pred"].grad_fn is None
    finally:
        model.duration_predictor.enable_backward(False)
    assert model.duration_predictor(enc).grad_fn is None


# ---- the gradients -----------------------------------------------------------------

@pytest.mark.parametrize("case", list(orc.CASES))
def test_gradients_match_float64_autograd(gpu, case):
    from m2amd import ops
    e = _expect(case, gpu)
    H, B, S, mods = orc.CASES[case]
    bar = 32.0 * max(e["s"], EPS)
    names = [n for n, _ in e["pred"].named_parameters()] + ["d_enc"]
    got, want = e["got"] + [e["got_enc"]], e["grads"] + [e["d_enc"]]
    assert len(got) == 11
    worst = 0.0
    for name, g, ref in zip(names, got, want):
        assert g.shape == ref.shape and g.dtype == torch.float32 and g.is_cuda, (case, name)
        err = _rel(g.cpu(), ref)
        worst = max(worst, err)
        assert err <= bar, (case, name, err, bar)
    print(f"{case}: worst rel max err {worst:.3e}, cpu float32 {e['s']:.3e}, bar {bar:.3e}")
    if "gamma" in mods:  # d gamma and d beta where gamma is 0 and where it is negative
        for blk in (0, 1):
            for which in (2, 3):
                g, ref = e["got"][4 * blk + which].cpu().double(), e["grads"][4 * blk + which]
                for c in (orc.GAMMA_ZERO, orc.GAMMA_NEG):
                    assert float(ref[c].abs()) > 0 and float(g[c].abs()) > 0, (case, blk, which, c)
                    assert float((g[c] - ref[c]).abs()) <= bar * float(ref.abs().max()), (case, blk, which, c)
            assert float(e["params"][4 * blk + 2][orc.GAMMA_ZERO]) == 0.0 and float(e["params"][4 * blk + 2][orc.GAMMA_NEG]) < 0
    if "extreme" in mods:  # the positions above softplus's threshold and far below it
        _, _, _, z = orc.forward(e["p64"], e["enc"].cpu().double(), e["positive"])
        z = z.detach()
        top = float(e["d_enc"].abs().max())
        for where in (z > 20, z < -30):
            assert int(where.sum()) > 0
            assert float((e["got_enc"].cpu().double() - e["d_enc"])[where].abs().max()) <= bar * top
            # a cotangent on those positions alone: g_z = d_dur there, sigmoid(z) d_dur (next to nothing) here
            # The bar is the rule's, with s taken for this cotangent: far below zero sigmoid(z) is exp(z), whose
            # relative error is z's absolute one, so CPU float32 deviates more here than over the whole case.
            dd = e["dd"].cpu() * where
            g64, de64, _, _ = orc.gradients(e["p64"], e["enc"].cpu().double(), dd.double())
            g32, de32, _, _ = orc.gradients(e["p32"], e["enc"].cpu(), dd)
            s_here = max(_rel(a, b) for a, b in zip(g32 + [de32], g64 + [de64]))
            ref, ref_enc, _, _ = orc.gradients(e["p64"], e["enc"].cpu().double(), dd.double(), e["positive"])
            d_enc, grads = ops.duration_backward(e["params"], e["bn"], e["enc"], e["tape"], dd.to(gpu))
            worst = max(_rel(g.cpu(), r) for g, r in zip(grads + [d_enc], ref + [ref_enc]))
            print(f"{case}: cotangent on {int(where.sum())} positions with z up to {float(z[where].max()):.1f}: "
                  f"worst {worst:.3e}, cpu float32 {s_here:.3e}")
            assert worst <= 32.0 * max(s_here, EPS), (case, float(z[where].max()))
        small = (e["dd"].cpu() * (z < -30)).double()
        _, ref_enc, _, _ = orc.gradients(e["p64"], e["enc"].cpu().double(), small, e["positive"])
        assert float(ref_enc.abs().max()) < 1e-9 * top


@pytest.mark.parametrize("case", ["s1", "edge63", "wide", "h24"])
def test_d_enc_does_not_depend_on_the_batch(gpu, case):
    from m2amd import ops
    e = _expect(case, gpu)
    B = orc.CASES[case][1]
    assert B > 1
    for b in range(B):
        enc = e["enc"][b:b + 1].contiguous()
        dur, tape = ops.duration_train_forward(e["params"], e["bn"], enc)
        assert torch.equal(dur[0], e["dur"][b])
        d_enc, _ = ops.duration_backward(e["params"], e["bn"], enc, tape, e["dd"][b:b + 1].contiguous(),
                                         need=[False] * 10)
        assert torch.equal(d_enc[0], e["got_enc"][b]), (case, b)


@pytest.mark.parametrize("case", ["s1", "one", "wide", "h24"])
def test_determinism_accumulation_and_need(gpu, case):
    from m2amd import ops
    e = _expect(case, gpu)
    args = (e["params"], e["bn"], e["enc"], e["tape"], e["dd"])
    d_enc, grads = ops.duration_backward(*args)
    assert len(grads) == 10 and all(torch.equal(a, b) for a, b in zip(grads, e["got"]))
    assert torch.equal(d_enc, e["got_enc"])
    g = torch.Generator().manual_seed(5)
    onto = [torch.randn(p.shape, generator=g).to(gpu) for p in e["params"]]
    before = [o.clone() for o in onto]
    d_again, twice = ops.duration_backward(*args, accumulate=onto)
    assert all(t is o for t, o in zip(twice, onto)) and torch.equal(d_again, e["got_enc"])
    assert all(torch.equal(t, b + g_) for t, b, g_ in zip(twice, before, grads))  # one fp32 addition per element
    need = [i % 3 != 1 for i in range(10)]
    _, some = ops.duration_backward(*args, need=need)
    for i, (g_, full) in enumerate(zip(some, e["got"])):
        assert (g_ is None) == (not need[i]) and (g_ is None or torch.equal(g_, full)), i
    none_enc, all_ = ops.duration_backward(*args, need_enc=False)
    assert none_enc is None and all(torch.equal(a, b) for a, b in zip(all_, e["got"]))
    only_enc, none = ops.duration_backward(*args, need=[False] * 10)
    assert torch.equal(only_enc, e["got_enc"]) and all(g_ is None for g_ in none)
    no_enc, head = ops.duration_backward(*args, need_enc=False, need=[False] * 4 + [True] * 6)  # block 1 is skipped
    assert no_enc is None and all(g_ is None for g_ in head[:4])
    assert all(torch.equal(a, b) for a, b in zip(head[4:], e["got"][4:]))
    _, gammas = ops.duration_backward(*args, need=[i in (2, 6) for i in range(10)])
    assert torch.equal(gammas[2], e["got"][2]) and torch.equal(gammas[6], e["got"][6])


def test_abi_conventions(gpu):
    from m2amd import _lib, ops
    lib = _lib.load()
    case = "edge63"
    e = _expect(case, gpu)
    H, B, S, _ = orc.CASES[case]
    pp = (ctypes.c_void_p * 10)(*[p.data_ptr() for p in e["params"]])
    outs = [torch.full_like(p, -1.0) for p in e["params"]]
    gp = (ctypes.c_void_p * 10)(*[g.data_ptr() for g in outs])
    dur = torch.full((B, S), -2.0, device=gpu)
    d_enc = torch.full((B, S, H), -3.0, device=gpu)
    tape_bytes = lib.m2_duration_tape_bytes(H, B, S)
    ws_bytes = lib.m2_duration_backward_workspace_bytes(H, B, S)
    tape = torch.empty(tape_bytes, dtype=torch.uint8, device=gpu)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=gpu)
    bn, enc, dd = e["bn"].data_ptr(), e["enc"].data_ptr(), e["dd"].data_ptr()
    fwd = lambda b, s, nbytes: lib.m2_duration_train_forward(pp, bn, H, enc, b, s, dur.data_ptr(),  # noqa: E731
                                                             tape.data_ptr(), nbytes, None)
    bwd = lambda b, s, nbytes: lib.m2_duration_backward(pp, bn, H, enc, b, s, e["tape"].data_ptr(), dd,  # noqa: E731
                                                        d_enc.data_ptr(), gp, 0, ws.data_ptr(), nbytes, None)
    assert fwd(B, S, tape_bytes - 512) == -1 and b"tape too small" in lib.m2_last_error()
    assert bwd(B, S, ws_bytes - 512) == -1 and b"workspace too small" in lib.m2_last_error()
    assert fwd(0, S, 0) == 0 and fwd(B, 0, 0) == 0 and bwd(0, S, 0) == 0 and bwd(B, 0, 0) == 0
    pp[5] = None
    assert fwd(B, S, tape_bytes) == -1 and bwd(B, S, ws_bytes) == -1
    pp[5] = e["params"][5].data_ptr()
    torch.cuda.synchronize()
    assert bool((dur == -2.0).all()) and bool((d_enc == -3.0).all()) and all(bool((g == -1.0).all()) for g in outs)
    assert fwd(B, S, tape_bytes) == 0 and bwd(B, S, ws_bytes) == 0  # the queried sizes are accepted
    torch.cuda.synchronize()
    assert torch.equal(dur, e["dur"]) and torch.equal(d_enc, e["got_enc"])
    assert all(torch.equal(g, w) for g, w in zip(outs, e["got"]))
    # the wrappers refuse a tape of another shape and arguments of the wrong form
    with pytest.raises(ValueError, match="tape"):
        ops.duration_backward(e["params"], e["bn"], e["enc"], e["tape"][:tape_bytes - 512], e["dd"])
    with pytest.raises(ValueError, match="d_dur"):
        ops.duration_backward(e["params"], e["bn"], e["enc"], e["tape"], e["dd"][:, :-1])
    with pytest.raises(ValueError, match="bn_stats"):
        ops.duration_train_forward(e["params"], e["bn"][:4], e["enc"])
    with pytest.raises(ValueError, match="parameters"):
        ops.duration_train_forward(e["params"][:8], e["bn"], e["enc"])
    with pytest.raises(ValueError, match="enc must be"):
        ops.duration_train_forward(e["params"], e["bn"], e["enc"][:, :, :-8])


# ---- the module --------------------------------------------------------------------

def _zero(params):
    for p in params:
        p.grad = None


def test_module_backward(gpu):
    e = _expect("s1", gpu)
    pred = copy.deepcopy(e["pred"])
    params = list(pred.parameters())
    enc, dd = e["enc"], e["dd"]
    assert all(p.requires_grad for p in params) and torch.is_grad_enabled()
    assert pred.backward_enabled is False and pred(enc).grad_fn is None  # the switch is off
    assert pred.enable_backward() is pred
    with torch.no_grad():
        assert pred(enc).grad_fn is None
    dur = pred(enc)
    assert dur.grad_fn is not None and torch.equal(dur.detach(), e["dur"])
    dur.backward(dd)
    assert all(torch.equal(p.grad, g) for p, g in zip(params, e["got"]))
    pred(enc).backward(dd)  # a second backward accumulates
    assert all(torch.equal(p.grad, 2.0 * g) for p, g in zip(params, e["got"]))
    _zero(params)
    leaf = enc.clone().requires_grad_()
    pred(leaf).backward(dd)
    assert torch.equal(leaf.grad, e["got_enc"]) and all(torch.equal(p.grad, g) for p, g in zip(params, e["got"]))
    with pytest.raises(RuntimeError):  # once differentiable
        (gw,) = torch.autograd.grad(pred(enc), params[:1], dd, create_graph=True)
        gw.sum().backward()
    # frozen parameters get None; the input's gradient alone
    frozen = [params[0], params[2], params[7], params[9]]
    for p in frozen:
        p.requires_grad_(False)
    _zero(params)
    pred(enc).backward(dd)
    assert all(p.grad is None for p in frozen)
    assert all(torch.equal(p.grad, g) for p, g in zip(params, e["got"]) if not any(p is f for f in frozen))
    for p in params:
        p.requires_grad_(False)
    assert pred(enc).grad_fn is None  # nothing requires grad: today's path
    leaf.grad = None
    _zero(params)
    pred(leaf).backward(dd)  # the input's gradient alone
    assert torch.equal(leaf.grad, e["got_enc"]) and all(p.grad is None for p in params)
    for p in params:
        p.requires_grad_(True)
    # the buffers are constants: neither a gradient nor a write, in training mode too
    from models import components
    buffers = {k: v.clone() for k, v in pred.named_buffers()}
    assert len(buffers) == 6 and any(k.endswith("num_batches_tracked") for k in buffers)
    pred.train()
    components._WARNED.discard("ConvBlock")
    with pytest.warns(RuntimeWarning, match="BatchNorm statistics are not applied"):
        trained = pred(enc)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pred(enc)  # once only
    assert trained.grad_fn is not None and torch.equal(trained.detach(), e["dur"])
    trained.backward(dd)
    pred.eval()
    assert all(torch.equal(v, buffers[k]) for k, v in pred.named_buffers())
    assert all(not v.requires_grad for v in pred.buffers())
    assert pred.enable_backward(False) is pred and pred(enc).grad_fn is None


def test_unsupported_shapes_raise(gpu):
    from m2amd import ops
    from models.tts_model import DurationPredictor
    for bad in (dict(hidden_dim=8), dict(hidden_dim=136), dict(hidden_dim=64, kernel_size=5)):
        pred = DurationPredictor(**bad).to(gpu)
        with pytest.raises(NotImplementedError):
            pred.enable_backward()
        assert pred.backward_enabled is False
        h = bad["hidden_dim"]
        with pytest.raises((ops.M2Error, ValueError)):
            ops.duration_train_forward(list(pred.parameters()), _bn_stats(pred), torch.zeros(1, 3, h, device=gpu))


def test_optimizer_step_matches_float64(gpu):
    """zero_grad, backward of sum(dur d_dur), SGD step on a model's duration predictor, and the next module
    call on the updated weights; the BatchNorm buffers stay as they were."""
    from models.tts_model import M2TTSModel
    e = _expect("s1", gpu)
    torch.manual_seed(32)
    model = M2TTSModel().to(gpu).eval()
    model.duration_predictor.load_state_dict(e["pred"].state_dict())
    model.duration_predictor.enable_backward()
    params = list(model.duration_predictor.parameters())
    buffers = {k: v.clone() for k, v in model.duration_predictor.named_buffers()}
    enc, dd = e["enc"], e["dd"]
    opt = torch.optim.SGD(params, lr=LR)
    opt.zero_grad()
    (model.duration_predictor(enc) * dd).sum().backward()
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
    assert float(params[2].detach()[orc.GAMMA_ZERO]) != 0.0  # the dead gamma came alive
    now = dict(model.duration_predictor.named_buffers())
    assert set(now) == set(buffers) and all(torch.equal(now[k], v) for k, v in buffers.items())
    assert all(int(v) == 0 for k, v in now.items() if k.endswith("num_batches_tracked"))
    after = model.duration_predictor(enc)
    alone = copy.deepcopy(model.duration_predictor).enable_backward(False)
    with torch.no_grad():
        want = alone(enc)
    assert after.grad_fn is not None and torch.equal(after.detach(), want)  # the updated weights are read
    assert not torch.equal(want, e["dur"])
    model.duration_predictor.enable_backward(False)
