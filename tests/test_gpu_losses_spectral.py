"""GPU: the gradient of the spectral and perceptual losses (m2_loss_spectral_backward,
Dsp.loss_spectral_backward, training.losses' spectral switch) against the float64 oracle of
tests/golden/losses_spectral_oracle.py.  Nothing here reads the reference.

Runs: lc.FULL_CASES at the three n_ffts (hop n_fft / 4); `short257`, B = 1, L = 257 at n_fft 512,
the shortest accepted, where both reflections cover the whole signal; `hop200`, B = 2, L = 777 at
n_fft 512 and hop 200, which does not divide n_fft (checks (a) and (b) only).  Every run has all
three coefficients on, at the values the losses use for that size.

(a) cotangent   The dumped cotangent equals the closed form in float64 on the spectra the GPU
                itself dumps (m2_loss_spectral(spectra=True), bit-equal to the backward's), per
                bin within 2^-22 |want|: both sides compute in double from the same float32
                inputs, one rounding to float is 2^-24 per component, and the bar leaves 2.
(b) adjoint     d_pred equals the float64 adjoint of the dumped cotangent per utterance within
                32 x 2e-6 x max|want|, the STFT bar on the transposed transform.
(c) end to end  d_pred against float64 autograd of the formula over torch.stft, with the GPU's
                signs prescribed: |g_gpu - g_f64| <= 32 x max(s, 2^-24) x max|g_f64|, s the
                deviation of CPU float32 autograd with the same signs from float64 (printed).
                Per run, and for SpectralLoss, PerceptualLoss and 1.0 x + 0.5 x their sum.
    sign caps   A sign taken from the GPU where float64 has another must be unresolvable: in a
                symmetric frame (frame 0; the last when L = 1 mod hop) both |im_f64| lie within
                the STFT bar 32 x 2e-6 x max|X|; in an ordinary frame |angle P - angle T| in
                float64 is at most bar_P / |P| + bar_T / |T|, or P or T lies within its bar of the
                negative real axis, and at most 1 bin in 10,000 per run differs.  Magnitude and
                perceptual signs agree exactly.  The counts are printed.
    module      total_loss.backward() at the default weights: audio_pred.grad against the
                generator step's d_fake plus the standalone gradients that the total adds to it,
                per sample within the rounding of its three fp32 additions,
                |got - sum of the terms| <= 3 x 2^-24 x sum |terms| of that sample.  The terms
                are d_fake and the total's three calls each run alone (n_fft 512, 1024 with the
                perceptual term and its weight, 2048), so that only the additions differ.  The
                spectral and the perceptual gradient as two separate tensors cannot be the
                terms of a per-sample bar: the total's 1024 call takes both through one fp32
                inverse FFT, they go through one each, and an FFT's rounding is relative to its
                frame, not to the sample (on `one` 78 of 1025 samples and on `edge41` 435 of
                5248 lie beyond 3 x 2^-24 x (|d_fake| + |spectral| + |perceptual|); the largest
                difference is 4.6e-9 and 1.2e-9 at max|gradient| 0.07 and 0.013).  That the three calls in one
                chain are the weighted sum of the two losses' gradients is checked against the
                float64 oracle with bar (c).
"""
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, str(GOLDEN))
import losses_cases as lc  # noqa: E402
import losses_spectral_oracle as sorc  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
STFT_BAR = 32 * 2e-6
EXTRA = {"short257": (1, 257, 257), "hop200": (2, 777, 200)}  # B, L, seed
RUNS = [(case, n_fft, n_fft // 4) for case in lc.FULL_CASES for n_fft in lc.N_FFTS] + \
    [("short257", 512, 128), ("hop200", 512, 200)]
END_TO_END = [r for r in RUNS if r[0] != "hop200"]
M2_OK, M2_E_ARG, M2_E_SHAPE, M2_E_WORKSPACE = 0, -1, -2, -3


def _id(run):
    return f"{run[0]}-{run[1]}-{run[2]}"


def _audio(case):
    """(pred, target) float32 numpy [B, L]."""
    if case in lc.CASES:
        pred, target = lc.audio_case(case)
        return pred[:, 0], target[:, 0]
    B, L, seed = EXTRA[case]
    rng = np.random.default_rng(seed)
    pre = 0.5 * rng.standard_normal((B, L))
    return (np.tanh(pre + 0.15 * rng.standard_normal((B, L))).astype(np.float32), np.tanh(pre).astype(np.float32))


def _dsp(gpu, n_fft, hop):
    from m2amd.dsp import get_dsp
    return get_dsp(lc.SR, n_fft, hop, n_fft, device=gpu)


def _weights(gpu, n_fft):
    from training.losses import PerceptualLoss
    w = PerceptualLoss.mel_weights(gpu, n_fft // 2 + 1)
    assert torch.equal(w.cpu(), sorc.mel_weights(n_fft // 2 + 1))
    return w


_GPU, _EXPECT = {}, {}


def _gpu_run(gpu, run):
    """Once per run: the GPU's spectra, cotangent and gradient (numpy), with the run's inputs."""
    if run in _GPU:
        return _GPU[run]
    case, n_fft, hop = run
    pred, target = _audio(case)
    B, L = pred.shape
    d, w = _dsp(gpu, n_fft, hop), _weights(gpu, n_fft)
    c = sorc.coefficients(B, L, n_fft, hop)
    p, t = torch.from_numpy(pred).to(gpu), torch.from_numpy(target).to(gpu)
    _, sp, st = d.loss_spectral(p, t, w, spectra=True)
    g, cot = d.loss_spectral_backward(p, t, w, *c, cotangent=True)
    assert g.shape == (B, L) and g.dtype == torch.float32 and g.is_cuda
    assert cot.shape == sp.shape == (B, n_fft // 2 + 1, 1 + L // hop) and cot.dtype == torch.complex64
    _GPU[run] = {"pred": pred, "target": target, "p": p, "t": t, "w": w, "c": c, "sp": sp.cpu().numpy(),
                 "st": st.cpu().numpy(), "cot": cot.cpu().numpy(), "grad": g.cpu().numpy()}
    return _GPU[run]


def _expect(gpu, run):
    """Once per run: the sign caps, and float64 / float32 autograd with the GPU's signs, the
    spectral pair of terms and the perceptual term apart."""
    if run in _EXPECT:
        return _EXPECT[run]
    case, n_fft, hop = run
    r = _gpu_run(gpu, run)
    w = r["w"].cpu().numpy()
    p64, t64 = torch.from_numpy(r["pred"]).double(), torch.from_numpy(r["target"]).double()
    P, T = sorc.stft(p64, n_fft, hop).numpy(), sorc.stft(t64, n_fft, hop).numpy()
    dev, own = sorc.signs_of(r["sp"], r["st"], w), sorc.signs_of(P, T, w)
    assert np.array_equal(dev[0], own[0]), (run, "a magnitude sign differs")
    assert np.array_equal(dev[2], own[2]), (run, "a perceptual sign differs")
    differ = dev[1] != own[1]
    bar_p = STFT_BAR * np.abs(P).max(axis=(1, 2), keepdims=True) * np.ones_like(P.real)
    bar_t = STFT_BAR * np.abs(T).max(axis=(1, 2), keepdims=True) * np.ones_like(T.real)
    sym = np.zeros(P.shape[2], dtype=bool)
    sym[lc.symmetric_frames(r["pred"].shape[1], hop)] = True
    in_sym, ordinary = differ & sym[None, None, :], differ & ~sym[None, None, :]
    assert np.all(np.abs(P.imag)[in_sym] <= bar_p[in_sym]) and np.all(np.abs(T.imag)[in_sym] <= bar_t[in_sym]), \
        (run, "a resolvable bin of a symmetric frame changed sign")
    delta = np.abs(np.angle(P) - np.angle(T))
    with np.errstate(divide="ignore"):
        close = delta <= bar_p / np.abs(P) + bar_t / np.abs(T)
    axis = ((P.real < 0) & (np.abs(P.imag) <= bar_p)) | ((T.real < 0) & (np.abs(T.imag) <= bar_t))
    assert np.all((close | axis)[ordinary]), (run, "a resolvable bin of an ordinary frame changed sign")
    n_ord = int((~sym).sum()) * P.shape[0] * P.shape[1]
    n_sym = int(sym.sum()) * P.shape[0] * P.shape[1]
    print(f"{_id(run)}: phase signs taken from the GPU: {int(in_sym.sum())} of {n_sym} bins of symmetric frames, "
          f"{int(ordinary.sum())} of {n_ord} bins of ordinary frames")
    assert int(ordinary.sum()) * 10000 <= n_ord, run
    c = r["c"]
    out = {}
    for name, ck in (("spectral", (c[0], c[1], 0.0)), ("perceptual", (0.0, 0.0, c[2]))):
        g64 = sorc.gradient(p64, t64, n_fft, hop, w, *ck, signs=dev).numpy()
        g32 = sorc.gradient(p64.float(), t64.float(), n_fft, hop, w, *ck, signs=dev).numpy().astype(np.float64)
        out[name] = (g64, g32)
    _EXPECT[run] = out
    return out


def _check(got, g64, g32, what):
    top = np.abs(g64).max()
    s = np.abs(g32 - g64).max() / top
    err, bar = np.abs(got.astype(np.float64) - g64).max() / top, 32.0 * max(s, EPS)
    print(f"{what}: rel max err {err:.3e}, s (cpu float32) {s:.3e}, bar {bar:.3e}")
    assert got.shape == g64.shape and err <= bar, (what, err, bar)


# ---- the kernels -----------------------------------------------------------------

@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_cotangent_matches_the_closed_form_on_the_dumped_spectra(gpu, run):
    r = _gpu_run(gpu, run)
    want = sorc.cotangent(r["sp"], r["st"], r["w"].cpu().numpy(), *r["c"])
    err = np.abs(r["cot"].astype(np.complex128) - want)
    ratio = float((err[want != 0] / np.abs(want[want != 0])).max())
    print(f"{_id(run)}: cotangent max |got - want| / |want| {ratio:.3e} (bar {2.0 ** -22:.3e}), max|want| "
          f"{np.abs(want).max():.3e}")
    assert np.abs(want).max() > 0 and np.all(err <= 2.0 ** -22 * np.abs(want))


@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_gradient_is_the_adjoint_of_the_dumped_cotangent(gpu, run):
    case, n_fft, hop = run
    r = _gpu_run(gpu, run)
    want = sorc.adjoint(r["cot"], n_fft, hop, r["pred"].shape[1])
    for b in range(want.shape[0]):
        top = np.abs(want[b]).max()
        err = np.abs(r["grad"][b].astype(np.float64) - want[b]).max() / top
        print(f"{_id(run)} utterance {b}: adjoint rel max err {err:.3e} (bar {STFT_BAR:.3e})")
        assert top > 0 and err <= STFT_BAR, (run, b)


@pytest.mark.parametrize("run", END_TO_END, ids=_id)
def test_gradient_matches_float64_autograd(gpu, run):
    r, exp = _gpu_run(gpu, run), _expect(gpu, run)
    g64 = exp["spectral"][0] + exp["perceptual"][0]
    g32 = exp["spectral"][1] + exp["perceptual"][1]
    _check(r["grad"], g64, g32, f"{_id(run)} all three terms")


@pytest.mark.parametrize("run", [("edge41", 512, 128), ("edge41", 2048, 512), ("hop200", 512, 200)], ids=_id)
def test_accumulate_and_determinism(gpu, run):
    case, n_fft, hop = run
    r = _gpu_run(gpu, run)
    d, p, t, w, c = _dsp(gpu, n_fft, hop), r["p"], r["t"], r["w"], r["c"]
    g = d.loss_spectral_backward(p, t, w, *c)
    assert torch.equal(g.cpu(), torch.from_numpy(r["grad"]))  # two runs, and with or without the dump
    old = torch.randn(g.shape, generator=torch.Generator().manual_seed(5)).to(gpu)
    acc = old.clone()
    assert d.loss_spectral_backward(p, t, w, *c, out=acc, accumulate=True) is acc
    assert torch.equal(acc, old + g)
    over = old.clone()
    d.loss_spectral_backward(p, t, w, *c, out=over)
    assert torch.equal(over, g)
    for b in range(p.shape[0]):  # a batched row is the row of the utterance alone, at the same coefficients
        assert torch.equal(d.loss_spectral_backward(p[b:b + 1], t[b:b + 1], w, *c)[0], g[b]), (run, b)


@pytest.mark.parametrize("n_fft", lc.N_FFTS)
def test_zero_and_degenerate_inputs(gpu, n_fft):
    r = _gpu_run(gpu, ("edge41", n_fft, n_fft // 4))
    d, p, t, w, c = _dsp(gpu, n_fft, n_fft // 4), r["p"], r["t"], r["w"], r["c"]
    sentinel = torch.full_like(p, 7.0)
    for what, args in (("zero coefficients", (p, t, w, 0.0, 0.0, 0.0)), ("pred == target", (t, t.clone(), w, *c)),
                       ("pred == 0", (torch.zeros_like(p), t, w, *c)), ("no weights", (t, t, None, *c))):
        out = sentinel.clone()
        g, cot = d.loss_spectral_backward(*args, out=out, cotangent=True)
        assert g is out and bool(torch.isfinite(g).all()) and bool((g == 0).all()), (n_fft, what)
        assert bool((torch.view_as_real(cot.contiguous()) == 0).all()), (n_fft, what)
    # no weights (NULL, 0) with c_perc on, differing signals: the perceptual sum is empty
    none = d.loss_spectral_backward(p, t, None, *c)
    assert bool((none != 0).any()) and torch.equal(none, d.loss_spectral_backward(p, t, w, c[0], c[1], 0.0))
    assert not torch.equal(none, torch.from_numpy(r["grad"]).to(gpu))  # the weights do count


def _equal_frames(pred, target, n_fft, hop):
    """[B, frames] bool: the windowed samples of the frame are the same float32 values on both sides."""
    win = torch.hann_window(n_fft, periodic=True)
    pad = [torch.nn.functional.pad(torch.from_numpy(x)[:, None], (n_fft // 2, n_fft // 2), mode="reflect")[:, 0]
           for x in (pred, target)]
    fp, ft = (x.unfold(1, n_fft, hop) * win for x in pad)
    return (fp == ft).all(dim=2).numpy()


def test_some_frames_equal(gpu):
    """pred == target on a stretch: the frames inside it get a zero cotangent (P = T there, which the
    paired FFT's two halves would not reproduce), every other frame the closed form on the dumped
    spectra, and d_pred is the adjoint of that cotangent."""
    n_fft, hop = 512, 128
    pred, target = _audio("edge41")
    pred = pred.copy()
    pred[0, :1300] = target[0, :1300]   # frames 0..8 of utterance 0; frame 9 reaches sample 1300
    pred[1, 900:2000] = target[1, 900:2000]  # frames in the middle of utterance 1
    B, L = pred.shape
    same = _equal_frames(pred, target, n_fft, hop)
    assert same.shape == (B, 1 + L // hop) and same[0, :9].all() and not same[0, 9:].any()
    assert same[1].any() and not same[1, 0] and not same[1, -1]
    d, w = _dsp(gpu, n_fft, hop), _weights(gpu, n_fft)
    c = sorc.coefficients(B, L, n_fft, hop)
    p, t = torch.from_numpy(pred).to(gpu), torch.from_numpy(target).to(gpu)
    _, sp, st = d.loss_spectral(p, t, w, spectra=True)
    g, cot = d.loss_spectral_backward(p, t, w, *c, cotangent=True)
    cot = cot.cpu().numpy()
    want = sorc.cotangent(sp.cpu().numpy(), st.cpu().numpy(), w.cpu().numpy(), *c)
    want[np.broadcast_to(same[:, None, :], want.shape)] = 0.0
    assert not cot[np.broadcast_to(same[:, None, :], cot.shape)].any()
    assert np.all(np.abs(cot.astype(np.complex128) - want) <= 2.0 ** -22 * np.abs(want))
    adj = sorc.adjoint(cot, n_fft, hop, L)
    for b in range(B):
        top = np.abs(adj[b]).max()
        assert top > 0 and np.abs(g[b].cpu().numpy().astype(np.float64) - adj[b]).max() <= STFT_BAR * top, b
    assert bool((g[0, :1300 - n_fft] == 0).all())  # samples that only equal frames reach


def test_workspace_and_errors(gpu):
    from m2amd import _lib
    lib = _lib.load()
    B, L, n_fft, hop = 2, 2000, 1024, 256
    assert _audio("edge41")[0].shape[1] >= L
    h = _dsp(gpu, n_fft, hop).handle
    need = lib.m2_loss_spectral_backward_workspace_bytes(h, B, L)
    assert need == B * (1 + L // hop) * n_fft * 4 + 256
    assert lib.m2_loss_spectral_backward_workspace_bytes(None, B, L) == 0
    x = torch.from_numpy(_audio("edge41")[0][:, :L].copy()).to(gpu)
    y = torch.from_numpy(_audio("edge41")[1][:, :L].copy()).to(gpu)
    ws = torch.empty(2 * need, dtype=torch.uint8, device=gpu)
    out = torch.full((B, L), -1.0, device=gpu)

    def call(stated, d=h, pred=x.data_ptr(), target=y.data_ptr(), b=B, n=L, o=out.data_ptr(), wp=ws.data_ptr()):
        return lib.m2_loss_spectral_backward(d, pred, target, b, n, None, 0, 1e-3, 1e-4, 0.0, 0, o, None, wp, stated,
                                             None)

    assert call(need - 257) == M2_E_WORKSPACE
    assert b"m2_loss_spectral_backward" in lib.m2_last_error() and b"workspace" in lib.m2_last_error()
    assert call(need, wp=None) == M2_E_WORKSPACE
    assert call(need, d=None) == M2_E_ARG and call(need, pred=None) == M2_E_ARG
    assert call(need, target=None) == M2_E_ARG and call(need, o=None) == M2_E_ARG
    assert call(need, n=n_fft // 2) == M2_E_SHAPE  # reflect padding needs more than n_fft / 2 samples
    assert call(need, b=65536) == M2_E_SHAPE
    assert call(0, b=0, wp=None) == M2_OK
    assert lib.m2_loss_spectral_backward(h, x.data_ptr(), y.data_ptr(), B, L, None, 3, 1e-3, 1e-4, 1e-3, 0,
                                         out.data_ptr(), None, ws.data_ptr(), need, None) == M2_E_ARG  # weights missing
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())  # nothing was launched
    assert call(need - 256) == M2_OK
    tight = out.clone()
    assert call(2 * need) == M2_OK
    assert bool((tight != -1.0).any()) and torch.equal(tight, out)
    with pytest.raises(RuntimeError, match="reflect padding"):
        _dsp(gpu, n_fft, hop).loss_spectral_backward(x[:, :512], y[:, :512], None, 1.0, 0.1, 0.0)
    with pytest.raises(ValueError):
        _dsp(gpu, n_fft, hop).loss_spectral_backward(x, y[:, :-1], None, 1.0, 0.1, 0.0)
    with pytest.raises(ValueError, match="accumulate"):
        _dsp(gpu, n_fft, hop).loss_spectral_backward(x, y, None, 1.0, 0.1, 0.0, accumulate=True)


# ---- the module ------------------------------------------------------------------

@pytest.fixture(scope="module")
def loss(gpu):
    from training.losses import CombinedTTSLoss
    torch.manual_seed(lc.WEIGHT_SEED)
    return CombinedTTSLoss().eval().to(gpu)


def _no_graph(v):
    return v.grad_fn is None and not v.requires_grad


def _pair(gpu, case):
    pred, target = lc.audio_case(case)
    return torch.from_numpy(pred).to(gpu), torch.from_numpy(target).to(gpu)


def _module_expectation(gpu, case, spectral, perceptual):
    g64 = g32 = 0.0
    for n_fft in lc.N_FFTS:
        exp = _expect(gpu, (case, n_fft, n_fft // 4))
        g64 = g64 + spectral * exp["spectral"][0]
        g32 = g32 + spectral * exp["spectral"][1]
        if n_fft == 1024:
            g64 = g64 + perceptual * exp["perceptual"][0]
            g32 = g32 + perceptual * exp["perceptual"][1]
    return g64[:, None], g32[:, None]


@pytest.mark.parametrize("case", lc.FULL_CASES)
def test_spectral_and_perceptual_modules(gpu, case):
    from training.losses import PerceptualLoss, SpectralLoss, _spectral_gradient, spectral_backward_calls
    pred, target = _pair(gpu, case)
    B, L = pred.shape[0], pred.shape[2]
    for module, weights in ((SpectralLoss(), (1.0, 0.0)), (PerceptualLoss(), (0.0, 1.0))):
        off = module(pred, target)
        assert _no_graph(off) and _no_graph(module(pred.clone().requires_grad_(), target))  # the switch is off
        assert module.enable_backward() is module
        assert _no_graph(module(pred, target))  # the input does not require grad
        with torch.no_grad():
            assert _no_graph(module(pred.clone().requires_grad_(), target))
        x, tt = pred.clone().requires_grad_(), target.clone().requires_grad_()
        v = module(x, tt)
        assert v.grad_fn is not None and v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda
        assert torch.equal(v.detach(), off)
        v.backward()
        assert tt.grad is None and x.grad.shape == x.shape and x.grad.dtype == torch.float32
        g = x.grad.clone()
        _check(g.cpu().numpy(), *_module_expectation(gpu, case, *weights), f"{case} {type(module).__name__}")
        (0.5 * module(x, tt)).backward()  # a second backward accumulates, grad_output multiplies on the device
        assert torch.equal(x.grad, g + 0.5 * g)
        with pytest.raises(RuntimeError):  # once differentiable
            (gx,) = torch.autograd.grad(module(x, tt), x, create_graph=True)
            gx.sum().backward()
        module.enable_backward(False)
        assert _no_graph(module(x, tt))
    # the weighted sum as CombinedTTSLoss's total forms it: three calls, the 1024 one carrying both
    calls = spectral_backward_calls(B, L, [512, 1024, 2048], 0.25, 1.0, 0.5)
    assert len(calls) == 3 and calls[1][4] != 0
    both = _spectral_gradient(pred, target, calls)
    _check(both.cpu().numpy()[:, None], *_module_expectation(gpu, case, 1.0, 0.5),
           f"{case} 1.0 spectral + 0.5 perceptual")
    s = SpectralLoss().enable_backward()
    x = pred.clone().requires_grad_()
    one = s.stft_loss(x, target, 1024)
    assert torch.equal(one.detach(), SpectralLoss().stft_loss(pred, target, 1024))
    one.backward()
    exp = _expect(gpu, (case, 1024, 256))["spectral"]
    _check(x.grad.cpu().numpy(), 3.0 * exp[0][:, None], 3.0 * exp[1][:, None], f"{case} stft_loss(1024)")


@pytest.mark.parametrize("case", ["one", "edge41"])
def test_combined_loss_with_the_spectral_switch(gpu, loss, case):
    from training.losses import _spectral_gradient, spectral_backward_calls
    preds = ("mel_pred", "duration_pred", "audio_pred")

    def inputs():
        kw = {k: (None if v is None else torch.from_numpy(v).to(gpu)) for k, v in lc.loss_case(case).items()}
        for k in preds:
            kw[k].requires_grad_()
        return kw

    graphs = {"plain": ("mel_loss", "duration_loss"),
              "spectral": ("mel_loss", "duration_loss", "spectral_loss", "perceptual_loss", "total_loss"),
              "off": ()}
    off = loss(**inputs())
    dis_off = loss(**inputs(), optimize_discriminator=True)
    assert all(_no_graph(v) for v in list(off.values()) + list(dis_off.values()))
    params = list(loss.get_discriminator_parameters())
    try:
        for mode, switch in (("plain", lambda: loss.enable_backward()),
                             ("spectral", lambda: loss.enable_backward(spectral=True)),
                             ("plain", lambda: loss.enable_backward()), ("off", lambda: loss.enable_backward(False))):
            assert switch() is loss
            got = loss(**inputs())
            assert list(got) == list(off)
            for k in got:
                assert torch.equal(got[k].detach(), off[k]), (mode, k)  # bit-equal with the switch on
                assert got[k].dim() == 0 and got[k].dtype == torch.float32 and got[k].device == gpu
                assert (got[k].grad_fn is not None) == (k in graphs[mode]), (mode, k)
            with torch.no_grad():
                assert all(_no_graph(v) for v in loss(**inputs()).values())
            plain_audio = inputs()
            plain_audio["audio_pred"] = plain_audio["audio_pred"].detach()
            quiet = loss(**plain_audio)  # the audio does not require grad: its three terms and the total stay plain
            assert all((quiet[k].grad_fn is not None) == (mode != "off" and k in ("mel_loss", "duration_loss"))
                       for k in quiet), mode
            dis = loss(**inputs(), optimize_discriminator=True)  # discriminator mode is untouched
            for k in dis:
                assert torch.equal(dis[k].detach(), dis_off[k]), k
                assert (dis[k].grad_fn is not None) == (mode != "off" and k in ("discriminator_loss", "total_loss")), k

        loss.enable_backward(spectral=True)
        # the standalone terms
        fake, real = inputs()["audio_pred"].detach(), inputs()["audio_target"]
        _, d_fake = loss.adversarial_loss.discriminator._handle(gpu).gen_step(real, fake, loss.adversarial_loss_weight,
                                                                            loss.feature_matching_weight)
        B, L = fake.shape[0], fake.shape[2]
        g_spec = loss.spectral_loss_weight * _spectral_gradient(
            fake, real, spectral_backward_calls(B, L, spectral_weight=1.0, perceptual_weight=0.0)).reshape(fake.shape)
        g_perc = loss.perceptual_loss_weight * _spectral_gradient(
            fake, real, spectral_backward_calls(B, L, spectral_weight=0.0, perceptual_weight=1.0)).reshape(fake.shape)
        assert (loss.spectral_loss_weight, loss.perceptual_loss_weight) == (1.0, 0.5)

        kw = inputs()
        got = loss(**kw)
        got["spectral_loss"].backward()  # alone: the audio only, and no discriminator parameter
        assert torch.equal(kw["audio_pred"].grad, g_spec)
        assert kw["mel_pred"].grad is None and kw["duration_pred"].grad is None
        assert all(p.grad is None for p in params)
        kw["audio_pred"].grad = None
        got["perceptual_loss"].backward()
        assert torch.equal(kw["audio_pred"].grad, 2.0 * g_perc)  # the entry is unweighted: 2 x 0.5
        kw["audio_pred"].grad = None

        got["total_loss"].backward()
        assert all(kw[k].grad is not None and kw[k].grad.shape == kw[k].shape for k in preds)
        assert all(p.grad is None for p in params)
        # d_fake plus the standalone gradients the total adds to it: its three calls, each run alone
        # (module docstring).  Per sample, the rounding of the three fp32 additions.
        calls = spectral_backward_calls(B, L, loss.spectral_loss.n_fft_list, loss.spectral_loss.hop_length_factor,
                                        loss.spectral_loss_weight, loss.perceptual_loss_weight)
        assert [c[:2] for c in calls] == [(512, 128), (1024, 256), (2048, 512)] and calls[1][4] != 0
        pieces = [_spectral_gradient(fake, real, [c]).reshape(fake.shape) for c in calls]
        terms = [t.double() for t in [d_fake] + pieces]
        want, size = sum(terms), sum(t.abs() for t in terms)
        err = (kw["audio_pred"].grad.double() - want).abs()
        bar = 3 * EPS * size
        worst = float((err / bar)[size > 0].max())
        print(f"{case} total_loss -> audio_pred: max over the samples of |got - sum of the terms| / "
              f"(3 x 2^-24 x sum|terms|) = {worst:.3f}")
        assert bool((err <= bar).all()), (case, worst)
        # and the calls run in one chain, without d_fake, are the weighted pair of standalone gradients'
        # calls: the chain the oracle checks in test_spectral_and_perceptual_modules
        chain = _spectral_gradient(fake, real, calls).reshape(fake.shape)
        assert torch.equal(chain, (pieces[0] + pieces[1]) + pieces[2])

        # the mel and duration gradients are those of the plain switch, bit for bit
        loss.enable_backward()
        kw2 = inputs()
        got2 = loss(**kw2)
        (loss.mel_loss_weight * got2["mel_loss"] + loss.duration_loss_weight * got2["duration_loss"]).backward()
        for k in ("mel_pred", "duration_pred"):
            assert torch.equal(kw[k].grad, kw2[k].grad), k
        assert kw2["audio_pred"].grad is None
    finally:
        loss.enable_backward(False)
