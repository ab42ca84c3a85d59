"""GPU: the backward of the discriminator step (m2_conv1d_strided_backward,
m2_disc_step, training.losses' enable_backward) against torch autograd on the
CPU in float64.  Nothing here reads the reference: the oracle is this module's
own nn.Conv1d stacks, deep-copied to the CPU (tests/golden/losses_backward_oracle.py).

No bar comes from the GPU's output.  Per tensor g:
    |g_gpu - g_f64| <= 32 x max(s, 2^-24) x max|g_f64|,
s the largest relative deviation, over the tensors of the case, of CPU float32
autograd from float64 autograd, computed here (32: the margin the STFT test
gives fp32 rounding, test_gpu_audio_features.py:40).

LeakyReLU kinks are accounted exactly.  A pre-activation within fp32 rounding
of 0 can take the other slope on the GPU, and one such element moves every
gradient upstream of it by far more than rounding.  The float64 oracle applies
each LeakyReLU as a product with a constant slope mask taken from the sign of
the GPU's feature map (discriminator(x)); wherever that sign differs from the
float64 pre-activation, |pre_f64| must be within the forward bar of the map,
32 x max(s_fwd, 2^-24) x max|map| (s_fwd: CPU float32 against float64 on that
map), and at most 8 elements per case may differ.  The count is printed.

The optimizer step compares float32 parameters after the update with the same
update done in float64: the gradient bar times the learning rate, plus the
rounding of the stored float32 parameter itself, 2^-24 x max|p| (half an ulp
of the largest element: the update is rounded once on the GPU).
"""
import ctypes
import json
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

sys.path.insert(0, str(GOLDEN))
import losses_backward_oracle as orc  # noqa: E402
import losses_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
KINK_CAP = 8
STEP_CASES = ("odd", "one", "edge41")
PREFIX = "adversarial_loss.discriminator.discriminators"
LR, CLIP = 0.05, 1.0


@pytest.fixture(scope="module")
def loss(gpu):
    from training.losses import CombinedTTSLoss
    torch.manual_seed(lc.WEIGHT_SEED)
    return CombinedTTSLoss().eval().to(gpu)


def _rel(a, b):
    return float((a.double() - b).abs().max()) / float(b.abs().max())


# ---- single layers ---------------------------------------------------------------

def _layer_inputs(layer):
    """Input lengths of discriminator layer `layer` over the scales of the edge41 and odd cases."""
    out = []
    for case in ("edge41", "odd"):
        L = lc.CASES[case][4]
        for s in lc.SCALES:
            n = L // s if layer == 0 else lc.layer_lengths(L, s)[layer - 1]
            if n not in out:
                out.append(n)
    return out


def _read(L, k, stride, pad):
    """Which of the L input positions any output reads."""
    read = torch.zeros(L, dtype=torch.bool)
    for t in range((L + 2 * pad - k) // stride + 1):
        read[max(0, t * stride - pad):max(0, min(L, t * stride - pad + k))] = True
    return read


def _backward_case(gpu, x, w, dy, stride, pad, groups, slope, what):
    from m2amd import ops

    def autograd(dtype):
        xx, ww = x.to(dtype).requires_grad_(), w.to(dtype).requires_grad_()
        b = torch.zeros(w.shape[0], dtype=dtype, requires_grad=True)
        y = F.conv1d(F.leaky_relu(xx, slope), ww, b, stride, pad, 1, groups)
        return torch.autograd.grad(y, (xx, ww, b), dy.to(dtype))

    want, single = autograd(torch.float64), autograd(torch.float32)
    got = ops.conv1d_strided_backward(x.to(gpu), w.to(gpu), dy.to(gpu), stride=stride, padding=pad, groups=groups,
                                      in_slope=slope)
    s = max(_rel(a, b) for a, b in zip(single, want))
    bar = 32.0 * max(s, EPS)
    for name, g, ref in zip(("dx", "dw", "db"), got, want):
        assert g.shape == ref.shape and g.dtype == torch.float32, (what, name)
        err = _rel(g.cpu(), ref)
        print(f"{what} {name}: rel max err {err:.3e}, cpu float32 {s:.3e}, bar {bar:.3e}")
        assert err <= bar, (what, name)
    unread = ~_read(x.shape[-1], w.shape[-1], stride, pad)
    assert bool((got[0].cpu()[:, :, unread] == 0).all()), what
    assert bool((want[0][:, :, unread] == 0).all())
    only = ops.conv1d_strided_backward(x.to(gpu), w.to(gpu), dy.to(gpu), stride=stride, padding=pad, groups=groups,
                                       in_slope=slope, need_dx=False, need_db=False)
    assert only[0] is None and only[2] is None and torch.equal(only[1], got[1]), what  # equal inputs, equal bits
    return int(unread.sum())


@pytest.mark.parametrize("layer", range(7))
def test_single_layer_gradients_match_float64_autograd(gpu, loss, layer):
    cin, cout, k, stride, pad, groups = lc.LAYERS[layer]
    w = loss.state_dict()[f"{PREFIX}.0.{2 * layer}.weight"].cpu()
    assert list(w.shape) == [cout, cin // groups, k]
    g = torch.Generator().manual_seed(300 + layer)
    lengths = _layer_inputs(layer) + [1]  # 1: a single output
    if stride > 1:
        lengths.append(103)  # (103 + 2 pad - k) % stride = 2
        assert (103 + 2 * pad - k) % stride != 0
    assert (1 + 2 * pad - k) // stride + 1 == 1
    for n in lengths:
        for slope in (0.2, 1.0):
            x = torch.randn(3, cin, n, generator=g)
            dy = torch.randn(3, cout, (n + 2 * pad - k) // stride + 1, generator=g)
            _backward_case(gpu, x, w, dy, stride, pad, groups, slope, f"layer {layer} L {n} slope {slope}")


@pytest.mark.parametrize("cin,cout,k,stride,pad,groups,n,unread", [
    (6, 10, 4, 3, 2, 2, 50, 0),     # not the discriminator's: one thread per dx sample, one workgroup per dw element
    (6, 10, 4, 3, 0, 2, 50, 1),     # (50 - 4) % 3 = 1: the last sample is never read
    (16, 16, 3, 2, 0, 1, 150, 1),   # on the MFMA, two column tiles, the last sample never read
    (16, 32, 2, 3, 0, 1, 200, 66),  # stride above k: every third sample is never read (a phase without taps)
    (36, 48, 7, 3, 5, 4, 70, 0),    # 12 outputs of 9 inputs per group: row tiles that straddle groups
    (24, 40, 5, 1, 2, 1, 6, 0),     # dense, 6 columns, partial row tiles
])
def test_other_geometries(gpu, cin, cout, k, stride, pad, groups, n, unread):
    g = torch.Generator().manual_seed(cin * 1000 + k)
    w = torch.randn(cout, cin // groups, k, generator=g) / (cin // groups * k) ** 0.5
    for slope in (0.2, 1.0):
        x = torch.randn(3, cin, n, generator=g)
        dy = torch.randn(3, cout, (n + 2 * pad - k) // stride + 1, generator=g)
        what = f"conv {cin}->{cout} k{k} s{stride} p{pad} g{groups} L {n} slope {slope}"
        assert _backward_case(gpu, x, w, dy, stride, pad, groups, slope, what) == unread


# ---- the step --------------------------------------------------------------------

_EXPECT = {}


def _expect(case, loss, gpu):
    """The float64 gradients with the GPU's side of every kink, their bar's s, and the kink count;
    computed once per case (the weights of `loss` are never changed)."""
    if case in _EXPECT:
        return _EXPECT[case]
    disc = loss.adversarial_loss.discriminator
    fake, real = (torch.from_numpy(a) for a in lc.audio_case(case))
    s64, s32 = orc.cpu_stacks(disc, torch.float64), orc.cpu_stacks(disc, torch.float32)
    _, g64, rm64, fm64 = orc.gradients(s64, disc.scales, real.double(), fake.double())
    _, g32, rm32, fm32 = orc.gradients(s32, disc.scales, real, fake)
    s = max(_rel(a, b) for a, b in zip(g32, g64))
    positive, cpu_kinks, total = [], 0, 0
    for x, m64, m32 in ((real, rm64, rm32), (fake, fm64, fm32)):
        _, feats = disc(x.to(gpu))
        positive.append([[f.cpu() > 0 for f in row] for row in feats])
        cpu_kinks += sum(int(((a > 0) != (b > 0)).sum()) for ra, rb in zip(m32, m64) for a, b in zip(ra, rb))
        total += sum(b.numel() for rb in m64 for b in rb)
    value, grads, rm, fm = orc.gradients(s64, disc.scales, real.double(), fake.double(), positive[0], positive[1])
    kinks = 0
    for pos, maps, own64, own32 in ((positive[0], rm, rm64, rm32), (positive[1], fm, fm64, fm32)):
        for sc in range(3):
            for l in range(6):
                pre = maps[sc][l]
                top = float(own64[sc][l].abs().max())
                s_fwd = float((own32[sc][l].double() - own64[sc][l]).abs().max()) / top
                differ = (pre > 0) != pos[sc][l]
                assert bool((pre.abs()[differ] <= 32.0 * max(s_fwd, EPS) * top).all()), \
                    (case, sc, l, "a resolvable pre-activation changed sign")
                kinks += int(differ.sum())
    print(f"{case}: {kinks} of {total} pre-activations take the other LeakyReLU slope on the GPU "
          f"(CPU float32: {cpu_kinks}); s = {s:.3e}")
    assert kinks <= KINK_CAP, case
    _EXPECT[case] = {"grads": grads, "s": s, "kinks": kinks, "value": float(value)}
    return _EXPECT[case]


def _check_grads(got, exp, what):
    assert len(got) == len(exp["grads"]) == 42
    bar = 32.0 * max(exp["s"], EPS)
    worst = 0.0
    for i, (g, ref) in enumerate(zip(got, exp["grads"])):
        assert g.shape == ref.shape and g.dtype == torch.float32 and g.is_cuda, (what, i)
        err = _rel(g.cpu(), ref)
        worst = max(worst, err)
        assert err <= bar, (what, i, err, bar)
    print(f"{what}: worst rel max err {worst:.3e}, bar {bar:.3e}")


def _audio(case, gpu):
    fake, real = (torch.from_numpy(a).to(gpu) for a in lc.audio_case(case))
    return real, fake


@pytest.mark.parametrize("case", STEP_CASES)
def test_step_matches_float64_autograd(gpu, loss, case):
    h = loss.adversarial_loss.discriminator._handle(gpu)
    real, fake = _audio(case, gpu)
    rows, grads = h.step(real, fake)
    assert torch.equal(rows, h.losses(real, fake))
    _check_grads(grads, _expect(case, loss, gpu), case)
    rows2, grads2 = h.step(real, fake)
    assert torch.equal(rows, rows2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))


def test_step_in_slices(gpu, loss):
    h = loss.adversarial_loss.discriminator._handle(gpu)
    real, fake = _audio("odd", gpu)
    rows, grads = h.step(real, fake)
    h.set_slice_bytes(1)  # one utterance per slice: three slices
    try:
        rows1, grads1 = h.step(real, fake)
        assert torch.equal(rows, rows1)
        _check_grads(grads1, _expect("odd", loss, gpu), "odd, one utterance per slice")
        again = h.step(real, fake)[1]
        assert all(torch.equal(a, b) for a, b in zip(grads1, again))
    finally:
        h.set_slice_bytes(0)
    assert all(torch.equal(a, b) for a, b in zip(grads, h.step(real, fake)[1]))


def test_step_abi_conventions(gpu, loss):
    from m2amd import _lib
    lib = _lib.load()
    h = loss.adversarial_loss.discriminator._handle(gpu).handle
    x = torch.zeros(2, 3000, device=gpu)
    out = torch.full((2, 64), -1.0, device=gpu, dtype=torch.float64)
    need = lib.m2_disc_step_workspace_bytes(h, 2, 3000)
    assert need > lib.m2_disc_losses_workspace_bytes(h, 2, 3000)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    ptrs = (ctypes.c_void_p * 42)(*[out.data_ptr()] * 42)
    args = (2, 3000, out.data_ptr(), ptrs, ws.data_ptr())
    assert lib.m2_disc_step(h, x.data_ptr(), x.data_ptr(), *args, 64, None) == -3  # M2_E_WORKSPACE
    assert lib.m2_disc_step(h, x.data_ptr(), None, *args, need, None) == -1  # both sides are required
    assert lib.m2_disc_step(h, None, x.data_ptr(), *args, need, None) == -1
    ptrs[17] = None
    assert lib.m2_disc_step(h, x.data_ptr(), x.data_ptr(), *args, need, None) == -1
    ptrs[17] = out.data_ptr()
    assert lib.m2_disc_step(h, x.data_ptr(), x.data_ptr(), 2, 3, out.data_ptr(), ptrs, ws.data_ptr(), need, None) == -2
    assert lib.m2_disc_step(h, x.data_ptr(), x.data_ptr(), 0, 3000, out.data_ptr(), ptrs, None, 0, None) == 0
    conv = (x.data_ptr(), x.data_ptr(), x.data_ptr())
    tail = (None, out.data_ptr(), None, ws.data_ptr())
    assert lib.m2_conv1d_strided_backward(*conv, 3, 1, 1, 4, 0.2, 2, 6, 6, 100, *tail, need, None) == -2  # groups
    assert lib.m2_conv1d_strided_backward(*conv, 3, 0, 1, 1, 0.2, 2, 6, 6, 100, *tail, need, None) == -1  # stride 0
    assert lib.m2_conv1d_strided_backward(*conv, 9, 1, 1, 1, 0.2, 2, 6, 6, 4, *tail, need, None) == -2  # k > L + 2 p
    assert lib.m2_conv1d_strided_backward(*conv, 41, 4, 20, 4, 0.2, 2, 64, 128, 100, *tail, 64, None) == -3
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())  # nothing was launched


# ---- the module ------------------------------------------------------------------

def _zero(params):
    for p in params:
        p.grad = None


def test_module_backward(gpu, loss):
    adv = loss.adversarial_loss
    disc = adv.discriminator
    params = list(disc.parameters())
    real, fake = _audio("odd", gpu)
    assert all(p.requires_grad for p in params) and torch.is_grad_enabled()
    off = adv.discriminator_loss(real, fake)
    assert off.grad_fn is None and not off.requires_grad
    kw = {k: (None if v is None else torch.from_numpy(v).to(gpu)) for k, v in lc.loss_case("one").items()}
    dis_off = loss(**kw, optimize_discriminator=True)
    gen_off = loss(**kw, optimize_discriminator=False)
    assert loss.enable_backward() is loss
    try:
        with torch.no_grad():
            assert adv.discriminator_loss(real, fake).grad_fn is None
            assert all(v.grad_fn is None for v in loss(**kw, optimize_discriminator=True).values())
        # discriminator_loss
        _zero(params)
        v = adv.discriminator_loss(real, fake)
        assert v.grad_fn is not None and v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda
        assert torch.equal(v.detach(), off)
        assert real.grad is None and fake.grad is None
        v.backward()
        g = [p.grad.clone() for p in params]
        _check_grads(g, _expect("odd", loss, gpu), "odd, discriminator_loss.backward()")
        adv.discriminator_loss(real, fake).backward()  # a second backward accumulates
        assert all(torch.equal(p.grad, 2.0 * a) for p, a in zip(params, g))
        _zero(params)
        (0.5 * adv.discriminator_loss(real, fake)).backward()
        assert all(torch.equal(p.grad, 0.5 * a) for p, a in zip(params, g))
        with pytest.raises(RuntimeError):  # once differentiable
            w = adv.discriminator_loss(real, fake)
            (gw,) = torch.autograd.grad(w, params[:1], create_graph=True)
            gw.sum().backward()
        # one scale frozen
        frozen = list(disc.discriminators[1].parameters())
        for p in frozen:
            p.requires_grad_(False)
        try:
            _zero(params)
            w = adv.discriminator_loss(real, fake)
            assert torch.equal(w.detach(), off)
            w.backward()
            assert all(p.grad is None for p in frozen)
            for i, (p, a) in enumerate(zip(params, g)):
                if not any(p is f for f in frozen):
                    assert torch.equal(p.grad, a), i
            assert sum(p.grad is not None for p in params) == 28
        finally:
            for p in frozen:
                p.requires_grad_(True)
        # CombinedTTSLoss on "one"
        real1, fake1 = _audio("one", gpu)
        _zero(params)
        adv.discriminator_loss(real1, fake1).backward()
        g1 = [p.grad.clone() for p in params]
        _check_grads(g1, _expect("one", loss, gpu), "one, discriminator_loss.backward()")
        _zero(params)
        dis = loss(**kw, optimize_discriminator=True)
        assert list(dis) == list(dis_off)
        for k in dis:
            assert torch.equal(dis[k].detach(), dis_off[k]), k
            assert (dis[k].grad_fn is not None) == (k in ("discriminator_loss", "total_loss")), k
            assert dis[k].dim() == 0 and dis[k].dtype == torch.float32 and dis[k].device == gpu
        dis["total_loss"].backward()
        assert all(torch.equal(p.grad, a) for p, a in zip(params, g1))
        gen = loss(**kw, optimize_discriminator=False)
        assert list(gen) == list(gen_off)
        for k in gen:
            assert gen[k].grad_fn is None and not gen[k].requires_grad and torch.equal(gen[k], gen_off[k]), k
        assert adv.generator_loss(fake).grad_fn is None and adv.feature_matching_loss(real, fake).grad_fn is None
        assert loss.enable_backward(False) is loss
        assert adv.discriminator_loss(real, fake).grad_fn is None
    finally:
        loss.enable_backward(False)
        _zero(params)


# ---- an optimizer step -----------------------------------------------------------

def test_optimizer_step_matches_float64(gpu, loss):
    """The reference trainer's sequence (train_stage2.py:269-295) with SGD: zero_grad, backward,
    clip_grad_norm_, step - and the next loss on the updated weights, which shows the repack."""
    ref = json.loads((GOLDEN / "losses_reference.json").read_text())
    spread = max(c[m]["spread"]["discriminator_loss"] for c in ref["cases"].values()
                 for m in ("generator", "discriminator", "no_audio", "adversarial")
                 if m in c and "discriminator_loss" in c[m]["spread"])
    exp = _expect("odd", loss, gpu)
    from training.losses import AdversarialLoss
    adv = AdversarialLoss().to(gpu)
    adv.load_state_dict(loss.adversarial_loss.state_dict())
    adv.enable_backward()
    params = list(adv.discriminator.parameters())
    assert all(torch.equal(p, q) for p, q in zip(params, loss.adversarial_loss.discriminator.parameters()))
    real, fake = _audio("odd", gpu)
    opt = torch.optim.SGD(params, lr=LR)
    opt.zero_grad()
    before = adv.discriminator_loss(real, fake)
    before.backward()
    torch.nn.utils.clip_grad_norm_(params, CLIP)
    opt.step()
    after = adv.discriminator_loss(real, fake)

    stacks = orc.cpu_stacks(loss.adversarial_loss.discriminator, torch.float64)
    p64 = orc.parameters(stacks)
    for p, g in zip(p64, exp["grads"]):
        p.grad = g.clone()
    norm = torch.nn.utils.clip_grad_norm_(p64, CLIP)
    assert float(norm) > CLIP  # the clipping acts
    torch.optim.SGD(p64, lr=LR).step()
    bar_g = 32.0 * max(exp["s"], EPS)
    for i, (p, q, g) in enumerate(zip(params, p64, exp["grads"])):
        err = float((p.detach().cpu().double() - q.detach()).abs().max())
        bar = LR * bar_g * float(g.abs().max()) + EPS * float(q.detach().abs().max())
        assert err <= bar, (i, err, bar)
    fake64, real64 = (torch.from_numpy(a).double() for a in lc.audio_case("odd"))
    with torch.no_grad():
        want = float(orc.discriminator_loss(stacks, adv.discriminator.scales, real64, fake64)[0])
    got, start = float(after.detach()), float(before.detach())
    bar = 32.0 * max(spread, EPS)
    print(f"discriminator_loss before {start!r}, after {got!r}, float64 after {want!r}, rel {abs(got - want) / want:.3e}, "
          f"bar {bar:.3e}")
    assert abs(start - exp["value"]) <= bar * exp["value"]
    assert abs(got - want) <= bar * want
    assert got < start
