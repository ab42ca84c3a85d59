"""GPU: the generator step's gradient through the discriminators
(m2_conv1d_audio_backward, m2_disc_gen_step, training.losses' generator side)
against torch autograd on the CPU in float64.  Nothing here reads the
reference: the oracle is this module's own nn.Conv1d stacks, deep-copied to the
CPU (tests/golden/losses_generator_oracle.py).

The bar is test_gpu_losses_backward.py's.  Per tensor g:
    |g_gpu - g_f64| <= 32 x max(s, 2^-24) x max|g_f64|,
s the relative deviation of CPU float32 autograd from float64 autograd,
computed here with the float64 run's LeakyReLU masks and feature-matching signs
prescribed to both, so that a kink flip between the two cannot loosen the bar.

Kinks are accounted exactly.  A pre-activation, or a difference f_fake - f_real,
within fp32 rounding of 0 can fall on the other side on the GPU, and one such
element moves the gradient by far more than rounding.  The float64 oracle takes
the GPU's side of every LeakyReLU on both sides' maps and of every
sign(f_fake - f_real), read from discriminator(x)'s features; wherever a side
differs from float64, the float64 quantity must be within the forward bar of
that map, 32 x max(s_fwd, 2^-24) x max|map| (the sum of both maps' bars for a
difference), and at most 8 elements per case may differ.  The count is printed.
CPU float32 against float64 differs in no element of either kind.
"""
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

sys.path.insert(0, str(GOLDEN))
import losses_backward_oracle as orc  # noqa: E402
import losses_cases as lc  # noqa: E402
import losses_generator_oracle as gorc  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
KINK_CAP = 8
CASES = ("odd", "one", "edge41")
WEIGHTS = ((1.0, 0.0), (0.0, 1.0), (0.25, 2.0))
K, PAD = 15, 7


@pytest.fixture(scope="module")
def loss(gpu):
    from training.losses import CombinedTTSLoss
    torch.manual_seed(lc.WEIGHT_SEED)
    return CombinedTTSLoss().eval().to(gpu)


def _rel(a, b):
    return float((a.double() - b).abs().max()) / float(b.abs().max())


def _check(got, exp, what):
    ref, bar = exp["grad"], 32.0 * max(exp["s"], EPS)
    assert got.shape == ref.shape and got.dtype == torch.float32 and got.is_cuda, what
    err = _rel(got.cpu(), ref)
    print(f"{what}: rel max err {err:.3e}, cpu float32 {exp['s']:.3e}, bar {bar:.3e}")
    assert err <= bar, (what, err, bar)


# ---- the audio kernel alone ------------------------------------------------------

@pytest.mark.parametrize("pool", [1, 2, 4])
def test_audio_kernel_matches_float64_autograd(gpu, loss, pool):
    from m2amd import ops
    w = loss.state_dict()["adversarial_loss.discriminator.discriminators.0.0.weight"].cpu()
    assert list(w.shape) == [64, 1, K]
    g = torch.Generator().manual_seed(500 + pool)
    short = K * pool - 1  # fewer pooled samples than taps: the dy row is shorter than one thread's window
    for L in (1001, 1025, 2624, short):
        B, Lp = 3, L // pool
        assert L != 2624 or (Lp > 256 and Lp % 256)  # more than one workgroup per row, and a partial one
        dy = torch.randn(B, 64, Lp, generator=g)

        def autograd(dtype):
            x = torch.zeros(B, 1, L, dtype=dtype, requires_grad=True)
            y = F.conv1d(F.avg_pool1d(x, pool) if pool > 1 else x, w.to(dtype), padding=PAD)
            return torch.autograd.grad(y, x, dy.to(dtype))[0]

        want, single = autograd(torch.float64), autograd(torch.float32)
        s = _rel(single, want)
        exp = {"grad": want, "s": s}
        tail = slice(Lp * pool, L)
        assert bool((want[:, :, tail] == 0).all())
        got = ops.conv1d_audio_backward(dy.to(gpu), w.to(gpu), L, padding=PAD, pool=pool)
        _check(got, exp, f"audio kernel pool {pool} L {L}")
        assert bool((got[:, :, tail] == 0).all()), (pool, L)  # the samples floor pooling dropped
        assert torch.equal(got, ops.conv1d_audio_backward(dy.to(gpu), w.to(gpu), L, padding=PAD, pool=pool))
        # accumulate: added to what is there, the dropped samples untouched
        base = torch.randn(B, 1, L, generator=g)
        acc = base.to(gpu)
        assert ops.conv1d_audio_backward(dy.to(gpu), w.to(gpu), L, padding=PAD, pool=pool, out=acc) is acc
        assert torch.equal(acc[:, :, tail].cpu(), base[:, :, tail]), (pool, L)
        live = slice(0, Lp * pool)
        assert torch.equal(acc[:, :, live], base.to(gpu)[:, :, live] + got[:, :, live]), (pool, L)
        assert pool == 1 or L == 2624 or L % pool  # floor pooling drops samples at the odd lengths


# ---- the step --------------------------------------------------------------------

_MAPS, _EXPECT = {}, {}


def _case_maps(case, loss, gpu):
    """Per case, once: the audio, the CPU stacks, the float64 and float32 maps with their own kinks,
    the GPU's side of every kink, and the count of kinks that differ (checked against the forward bar)."""
    if case in _MAPS:
        return _MAPS[case]
    disc = loss.adversarial_loss.discriminator
    fake, real = (torch.from_numpy(a) for a in lc.audio_case(case))
    s64, s32 = orc.cpu_stacks(disc, torch.float64), orc.cpu_stacks(disc, torch.float32)
    with torch.no_grad():
        _, rm64 = orc.forward(s64, disc.scales, real.double())
        _, fm64 = orc.forward(s64, disc.scales, fake.double())
        _, rm32 = orc.forward(s32, disc.scales, real)
        _, fm32 = orc.forward(s32, disc.scales, fake)
        gr = disc(real.to(gpu))[1]
        gf = disc(fake.to(gpu))[1]
    gr, gf = [[m.cpu() for m in row] for row in gr], [[m.cpu() for m in row] for row in gf]
    own = {"pos_r": gorc.masks(rm64), "pos_f": gorc.masks(fm64), "sg": gorc.signs_of(fm64, rm64, torch.float64)}
    dev = {"pos_r": gorc.masks(gr), "pos_f": gorc.masks(gf), "sg": gorc.signs_of(gf, gr, torch.float64)}
    sg32 = gorc.signs_of(fm32, rm32, torch.float64)
    cpu_kinks = gpu_kinks = gpu_signs = total = 0
    for sc in range(3):
        for l in range(6):
            bars = []
            for m64, m32, pos in ((rm64[sc][l], rm32[sc][l], dev["pos_r"][sc][l]),
                                  (fm64[sc][l], fm32[sc][l], dev["pos_f"][sc][l])):
                top = float(m64.abs().max())
                s_fwd = float((m32.double() - m64).abs().max()) / top
                bars.append(32.0 * max(s_fwd, EPS) * top)
                differ = (m64 > 0) != pos
                assert bool((m64.abs()[differ] <= bars[-1]).all()), (case, sc, l, "a resolvable pre-activation changed sign")
                gpu_kinks += int(differ.sum())
                cpu_kinks += int(((m32 > 0) != (m64 > 0)).sum())
                total += m64.numel()
            differ = dev["sg"][sc][l] != own["sg"][sc][l]
            d64 = (fm64[sc][l] - rm64[sc][l]).abs()
            assert bool((d64[differ] <= bars[0] + bars[1]).all()), (case, sc, l, "a resolvable difference changed sign")
            gpu_signs += int(differ.sum())
            cpu_kinks += int((sg32[sc][l] != own["sg"][sc][l]).sum())
    print(f"{case}: on the GPU {gpu_kinks} of {total} pre-activations take the other LeakyReLU slope and "
          f"{gpu_signs} of {total // 2} differences the other sign (CPU float32: {cpu_kinks} of both kinds)")
    assert gpu_kinks + gpu_signs <= KINK_CAP, case
    assert cpu_kinks == 0, case
    _MAPS[case] = {"real": real, "fake": fake, "s64": s64, "s32": s32, "own": own, "dev": dev, "scales": disc.scales}
    return _MAPS[case]


def _expect(case, weights, loss, gpu):
    """The float64 gradient with the GPU's side of every kink and the bar's s, once per (case, weights)."""
    key = (case, weights)
    if key in _EXPECT:
        return _EXPECT[key]
    m = _case_maps(case, loss, gpu)
    w_adv, w_fm = weights
    real = m["real"] if w_fm else None
    r64 = None if real is None else real.double()
    own, dev = m["own"], m["dev"]
    sg32 = [[t.float() for t in row] for row in own["sg"]]
    _, g64, _, _ = gorc.gradient(m["s64"], m["scales"], r64, m["fake"].double(), w_adv, w_fm, own["pos_r"],
                                 own["pos_f"], own["sg"])
    _, g32, _, _ = gorc.gradient(m["s32"], m["scales"], real, m["fake"], w_adv, w_fm, own["pos_r"], own["pos_f"], sg32)
    value, grad, _, _ = gorc.gradient(m["s64"], m["scales"], r64, m["fake"].double(), w_adv, w_fm, dev["pos_r"],
                                      dev["pos_f"], dev["sg"])
    s = _rel(g32, g64)
    print(f"{case} weights {weights}: s = {s:.3e}")
    _EXPECT[key] = {"grad": grad, "s": s, "value": float(value)}
    return _EXPECT[key]


def _audio(case, gpu):
    fake, real = (torch.from_numpy(a).to(gpu) for a in lc.audio_case(case))
    return real, fake


@pytest.mark.parametrize("case", CASES)
def test_gen_step_matches_float64_autograd(gpu, loss, case):
    h = loss.adversarial_loss.discriminator._handle(gpu)
    real, fake = _audio(case, gpu)
    got = {}
    for weights in WEIGHTS:
        r = real if weights[1] else None
        rows, d_fake = h.gen_step(r, fake, *weights)
        assert torch.equal(rows, h.losses(r, fake)), (case, weights)
        _check(d_fake, _expect(case, weights, loss, gpu), f"{case} gen_step{weights}")
        rows2, again = h.gen_step(r, fake, *weights)
        assert torch.equal(rows, rows2) and torch.equal(d_fake, again), (case, weights)
        got[weights] = d_fake
    # real given with a zero feature-matching weight: both sides' rows, the adversarial gradient's bits
    rows, d_fake = h.gen_step(real, fake, 1.0, 0.0)
    assert torch.equal(rows, h.losses(real, fake)) and torch.equal(d_fake, got[(1.0, 0.0)])
    # linear in the weights, up to the summation order
    combined = 0.25 * got[(1.0, 0.0)] + 2.0 * got[(0.0, 1.0)]
    _check(combined, _expect(case, (0.25, 2.0), loss, gpu), f"{case} 0.25 (1, 0) + 2 (0, 1)")


def test_sign_of_zero_is_zero(gpu, loss):
    h = loss.adversarial_loss.discriminator._handle(gpu)
    _, fake = _audio("odd", gpu)
    rows, d_fake = h.gen_step(fake, fake.clone(), 0.0, 1.0)
    assert bool((d_fake == 0).all())
    assert torch.equal(rows, h.losses(fake, fake))


def test_gen_step_in_slices(gpu, loss):
    h = loss.adversarial_loss.discriminator._handle(gpu)
    real, fake = _audio("odd", gpu)
    rows, d_fake = h.gen_step(real, fake, 0.25, 2.0)
    h.set_slice_bytes(1)  # one utterance per slice: three slices
    try:
        rows1, d1 = h.gen_step(real, fake, 0.25, 2.0)
        assert torch.equal(rows, rows1)
        assert torch.equal(d_fake, d1)  # no kernel of the chain reduces over the batch
    finally:
        h.set_slice_bytes(0)
    assert torch.equal(d_fake, h.gen_step(real, fake, 0.25, 2.0)[1])


def test_gen_step_abi_conventions(gpu, loss):
    from m2amd import _lib
    lib = _lib.load()
    h = loss.adversarial_loss.discriminator._handle(gpu).handle
    x = torch.zeros(2, 3000, device=gpu)
    out = torch.full((2, 3000), -1.0, device=gpu, dtype=torch.float64)  # rows and d_fake both fit
    need = lib.m2_disc_gen_step_workspace_bytes(h, 2, 3000)
    assert lib.m2_disc_losses_workspace_bytes(h, 2, 3000) < need < lib.m2_disc_step_workspace_bytes(h, 2, 3000)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    xp, op, wp = x.data_ptr(), out.data_ptr(), ws.data_ptr()
    assert lib.m2_disc_gen_step(h, xp, xp, 2, 3000, 0.25, 2.0, op, op, wp, 64, None) == -3  # M2_E_WORKSPACE
    assert lib.m2_disc_gen_step(h, None, xp, 2, 3000, 0.25, 2.0, op, op, wp, need, None) == -1  # w_fm needs real
    assert b"m2_disc_gen_step" in lib.m2_last_error()
    assert lib.m2_disc_gen_step(h, xp, None, 2, 3000, 0.25, 2.0, op, op, wp, need, None) == -1
    assert lib.m2_disc_gen_step(h, xp, xp, 2, 3000, 0.25, 2.0, op, None, wp, need, None) == -1
    assert lib.m2_disc_gen_step(h, xp, xp, 2, 3000, 0.25, 2.0, None, op, wp, need, None) == -1
    assert lib.m2_disc_gen_step(h, xp, xp, 2, 3, 0.25, 2.0, op, op, wp, need, None) == -2  # below the largest scale
    assert lib.m2_disc_gen_step(h, xp, xp, 0, 3000, 0.25, 2.0, op, op, None, 0, None) == 0  # B == 0
    assert lib.m2_conv1d_audio_backward(xp, xp, K, PAD, 4, 2, 64, 3, 0, op, None) == -2
    assert lib.m2_conv1d_audio_backward(xp, xp, K, PAD, 1, 0, 64, 100, 0, op, None) == 0
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())  # nothing was launched


# ---- the module ------------------------------------------------------------------

def _no_graph(v):
    return v.grad_fn is None and not v.requires_grad


def test_module_generator_side(gpu, loss):
    adv = loss.adversarial_loss
    params = list(adv.discriminator.parameters())
    real, fake = _audio("odd", gpu)
    w = (0.25, 2.0)
    calls = {(1.0, 0.0): lambda f: adv.generator_loss(f), (0.0, 1.0): lambda f: adv.feature_matching_loss(real, f),
             w: lambda f: adv.generator_terms(real, f, *w)}
    off = {k: fn(fake) for k, fn in calls.items()}
    assert all(_no_graph(v) for v in off.values())
    assert all(_no_graph(fn(fake.clone().requires_grad_())) for fn in calls.values())  # the switch is off
    assert torch.equal(adv.generator_terms(real, fake), adv.generator_terms(real, fake, 1.0, 1.0))
    loss.enable_backward()
    try:
        assert all(_no_graph(fn(fake)) for fn in calls.values())  # the input does not require grad
        with torch.no_grad():
            assert all(_no_graph(fn(fake.clone().requires_grad_())) for fn in calls.values())
        for weights, fn in calls.items():
            x = fake.clone().requires_grad_()
            v = fn(x)
            assert v.grad_fn is not None and v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda, weights
            assert torch.equal(v.detach(), off[weights]), weights
            v.backward()
            g = x.grad.clone()
            _check(g, _expect("odd", weights, loss, gpu), f"odd, module {weights}")
            fn(x).backward()  # a second backward accumulates
            assert torch.equal(x.grad, 2.0 * g), weights
            x.grad = None
            (0.5 * fn(x)).backward()
            assert torch.equal(x.grad, 0.5 * g), weights
            with pytest.raises(RuntimeError):  # once differentiable
                (gx,) = torch.autograd.grad(fn(x), x, create_graph=True)
                gx.sum().backward()
            assert real.grad is None and all(p.grad is None for p in params), weights
        r = real.clone().requires_grad_()  # real never gets a gradient
        x = fake.clone().requires_grad_()
        adv.generator_terms(r, x, *w).backward()
        assert r.grad is None and x.grad is not None
    finally:
        loss.enable_backward(False)
    assert _no_graph(adv.generator_loss(fake.clone().requires_grad_()))


def _combined_reference(kw, loss, gpu, case, dtype=torch.float64):
    """float64 autograd of the reference's formulas for the terms CombinedTTSLoss(spectral 0, perceptual 0)
    sums, the adversarial pair with the GPU's kinks: the gradients of mel_pred, duration_pred, audio_pred."""
    mel = kw["mel_pred"].detach().cpu().to(dtype).requires_grad_()
    dur = kw["duration_pred"].detach().cpu().to(dtype).requires_grad_()
    target = kw["mel_target"].cpu().to(dtype).transpose(1, 2)
    if kw["mel_lengths"] is not None:
        mel_loss = 0
        for i in range(mel.shape[0]):
            n = min(int(kw["mel_lengths"][i]), mel.shape[1], target.shape[1])
            mel_loss = mel_loss + F.l1_loss(mel[i, :n], target[i, :n])
        mel_loss = mel_loss / mel.shape[0]
    else:
        mel_loss = F.l1_loss(mel, target)
    dur_loss = F.mse_loss(dur, kw["duration_target"].cpu().to(dtype))
    total = loss.mel_loss_weight * mel_loss + loss.duration_loss_weight * dur_loss
    g_mel, g_dur = torch.autograd.grad(total, (mel, dur))
    return g_mel, g_dur


@pytest.mark.parametrize("case", ["one", "edge41"])
def test_combined_loss_backward(gpu, loss, case):
    from training.losses import CombinedTTSLoss
    plain = CombinedTTSLoss(spectral_loss_weight=0, perceptual_loss_weight=0).eval().to(gpu)
    plain.load_state_dict(loss.state_dict())
    preds = ("mel_pred", "duration_pred", "audio_pred")

    def inputs():
        kw = {k: (None if v is None else torch.from_numpy(v).to(gpu)) for k, v in lc.loss_case(case).items()}
        for k in preds:
            kw[k].requires_grad_()
        return kw

    weights = (plain.adversarial_loss_weight, plain.feature_matching_weight)
    assert weights == (0.25, 2.0)
    exp = _expect(case, weights, loss, gpu)
    for module, whole in ((plain, True), (loss, False)):  # loss: the default weights, spectral and perceptual on
        off = module(**inputs())
        dis_off = module(**inputs(), optimize_discriminator=True)
        assert all(_no_graph(v) for v in list(off.values()) + list(dis_off.values()))
        module.enable_backward()
        try:
            kw = inputs()
            got = module(**kw)
            assert list(got) == list(off)
            for k in got:
                assert torch.equal(got[k].detach(), off[k]), k
                assert got[k].dim() == 0 and got[k].dtype == torch.float32 and got[k].device == gpu
                graph = k in ("mel_loss", "duration_loss") or (whole and k == "total_loss")
                assert (got[k].grad_fn is not None) == graph, k
            g_mel, g_dur = _combined_reference(kw, module, gpu, case)
            if whole:
                got["total_loss"].backward()
                _check(kw["audio_pred"].grad, exp, f"{case} total_loss -> audio_pred")
                _check(kw["mel_pred"].grad, {"grad": g_mel, "s": 0.0}, f"{case} total_loss -> mel_pred")
                _check(kw["duration_pred"].grad, {"grad": g_dur, "s": 0.0}, f"{case} total_loss -> duration_pred")
                lengths = lc.loss_case(case)["mel_lengths"]
                if lengths is not None:
                    assert tuple(lengths) == (12, 7)
                    for b, n in enumerate(lengths):
                        assert bool((kw["mel_pred"].grad[b, int(n):] == 0).all()), b
                        assert bool((kw["mel_pred"].grad[b, :int(n)] != 0).any()), b
            else:
                (module.mel_loss_weight * got["mel_loss"] + module.duration_loss_weight * got["duration_loss"]).backward()
                _check(kw["mel_pred"].grad, {"grad": g_mel, "s": 0.0}, f"{case} mel_loss -> mel_pred")
                _check(kw["duration_pred"].grad, {"grad": g_dur, "s": 0.0}, f"{case} duration_loss -> duration_pred")
                assert kw["audio_pred"].grad is None
            assert all(p.grad is None for p in module.get_discriminator_parameters())
            # discriminator mode is untouched: only the discriminator step's two entries carry a graph
            dis = module(**inputs(), optimize_discriminator=True)
            assert list(dis) == list(dis_off)
            for k in dis:
                assert torch.equal(dis[k].detach(), dis_off[k]), k
                assert (dis[k].grad_fn is not None) == (k in ("discriminator_loss", "total_loss")), k
        finally:
            module.enable_backward(False)
