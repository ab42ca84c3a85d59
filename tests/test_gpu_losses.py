"""GPU: the drop-in training.losses module (reference src/training/losses.py)
against the reference's own code, recorded in tests/golden/losses_reference.json
by tests/golden/make_losses_golden.py, and against torch on the CPU in float64.

No bar comes from the GPU's output; 32 is the margin the STFT test gives fp32
rounding (test_gpu_audio_features.py:40).

  single layers   m2_conv1d_strided against F.conv1d on the CPU in float64:
                  32 x max(s, 2^-24) x max|y_f64|, s the relative max deviation
                  of the CPU float32 F.conv1d, computed here.
  discriminator   logits, 256 samples and the mean |.| of each feature map
                  against the recorded float64 values, same form: s is the
                  deviation of this module's nn.Conv1d stack run by torch on
                  the CPU in float32, relative to the recorded max |.| of the map.
  scalars         against the recorded float64 value, relative, 32 x max(
                  recorded spread of the reference's float32 from its float64
                  evaluation over the cases, 2^-24).
  spectral term   accounted exactly.  With reflect padding frame 0 of every
                  torch.stft is symmetric about its centre, its imaginary
                  parts are rounding residue, and where re < 0 the angle is
                  +pi or -pi by the residue's sign; a few bins of other frames
                  lie nearer the negative real axis than a float32 STFT
                  resolves.  No implementation matches the reference's value to
                  fp32 rounding there.  So: (1) the spectra the kernel took its
                  sums from match torch.stft in float64 per bin within
                  32 x 2e-6 x max|X| of the utterance (the STFT bar); (2) the
                  kernel's sums equal the formula in float64 on those spectra
                  within 32 x 2^-24; (3) the loss equals the formula in float64
                  on the float64 spectra with, in every bin with re < 0 whose
                  im differs in sign between GPU and float64 (a flip), the sign
                  of im taken from the GPU - within 32 x max(the case's recorded
                  spread, 2^-24), the spread taken with the imaginary parts of
                  frame 0 (and of the last frame where it is symmetric too,
                  L = 1 mod hop) forced to +0 in both precisions; (4) every flipped bin
                  has |im_f64| within the per-bin bar of (1).  The flip counts
                  and the reference's raw value are printed.
"""
import json
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, golden

sys.path.insert(0, str(GOLDEN))
import losses_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

REF = json.loads((GOLDEN / "losses_reference.json").read_text())
REF_ARRAYS = golden("losses_reference")  # float64 logits and sampled feature values
EPS = 2.0 ** -24
WEIGHTS = {"mel_loss": 1.0, "duration_loss": 0.1, "spectral_loss": 1.0, "perceptual_loss": 0.5,
           "generator_loss": 0.25, "feature_matching_loss": 2.0}
PREFIX = "adversarial_loss.discriminator.discriminators"


@pytest.fixture(scope="module")
def cpu_loss():
    """The seeded module on the CPU (torch runs its nn.Conv1d stacks there in float32)."""
    from training.losses import CombinedTTSLoss
    torch.manual_seed(lc.WEIGHT_SEED)
    return CombinedTTSLoss().eval()


@pytest.fixture(scope="module")
def loss(gpu):
    from training.losses import CombinedTTSLoss
    torch.manual_seed(lc.WEIGHT_SEED)
    return CombinedTTSLoss().eval().to(gpu)


def _kw(name, dev):
    return {k: (None if v is None else torch.from_numpy(v).to(dev)) for k, v in lc.loss_case(name).items()}


def _bar(metric, modes=("generator", "discriminator", "no_audio", "adversarial")):
    s = 0.0
    for c in REF["cases"].values():
        for mode in modes:
            if mode in c and metric in c[mode]["spread"]:
                s = max(s, c[mode]["spread"][metric])
    return 32.0 * max(s, EPS)


def _check_scalar(got, want, metric, what, **kw):
    err, bar = abs(got - want) / abs(want), _bar(metric, **kw)
    print(f"{what} {metric}: got {got!r} f64 {want!r} rel {err:.3e} bar {bar:.3e}")
    assert err <= bar, (what, metric, got, want)


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


def _conv_case(gpu, x, w, b, stride, pad, groups, slope, what):
    from m2amd import ops
    want = F.leaky_relu(F.conv1d(x.double(), w.double(), b.double(), stride, pad, 1, groups), slope)
    single = F.leaky_relu(F.conv1d(x, w, b, stride, pad, 1, groups), slope)
    got = ops.conv1d_strided(x.to(gpu), w.to(gpu), b.to(gpu), stride=stride, padding=pad, groups=groups,
                             leaky_slope=slope).cpu()
    assert got.shape == want.shape, what
    top = float(want.abs().max())
    s = float((single.double() - want).abs().max()) / top
    err = float((got.double() - want).abs().max()) / top
    print(f"{what}: rel max err {err:.3e}, cpu float32 {s:.3e}, bar {32 * max(s, EPS):.3e}")
    assert err <= 32.0 * max(s, EPS), what


@pytest.mark.parametrize("layer", range(7))
def test_single_layer_matches_float64_conv(gpu, cpu_loss, layer):
    cin, cout, k, stride, pad, groups = lc.LAYERS[layer]
    sd = cpu_loss.state_dict()
    w, b = sd[f"{PREFIX}.0.{2 * layer}.weight"], sd[f"{PREFIX}.0.{2 * layer}.bias"]
    assert list(w.shape) == [cout, cin // groups, k]
    g = torch.Generator().manual_seed(100 + layer)
    for n in _layer_inputs(layer):
        x = torch.randn(2, cin, n, generator=g)
        _conv_case(gpu, x, w, b, stride, pad, groups, 0.2, f"layer {layer} L {n}")


@pytest.mark.parametrize("cin,cout,k,stride,pad,groups,n", [
    (24, 40, 5, 1, 2, 1, 6),     # dense, 6 columns, 40 rows: partial row and column tiles
    (16, 16, 3, 2, 0, 1, 150),   # no padding, stride 2, two position tiles
    (36, 48, 7, 3, 5, 4, 70),    # 12 outputs of 9 inputs per group: row tiles that straddle groups
    (6, 8, 9, 2, 4, 2, 33),      # fewer than 16 outputs: one thread per output
])
def test_other_conv_geometries(gpu, cin, cout, k, stride, pad, groups, n):
    g = torch.Generator().manual_seed(cin * 1000 + k)
    x = torch.randn(3, cin, n, generator=g)
    w, b = torch.randn(cout, cin // groups, k, generator=g) / (cin // groups * k) ** 0.5, torch.randn(cout, generator=g)
    _conv_case(gpu, x, w, b, stride, pad, groups, 1.0, f"conv {cin}->{cout} k{k} s{stride} g{groups} L {n}")


def test_avg_pool_drops_the_tail(gpu):
    from m2amd import ops
    x = torch.randn(3, 2, 1001, generator=torch.Generator().manual_seed(5))
    for k in (2, 4, 7):
        got, want = ops.avg_pool1d(x.to(gpu), k).cpu(), F.avg_pool1d(x.double(), k, k)
        assert got.shape == want.shape == (3, 2, 1001 // k)
        assert float((got.double() - want).abs().max()) <= 32 * EPS * float(want.abs().max())


# ---- the discriminators ----------------------------------------------------------

def test_seeded_weights_match_the_recorded_fingerprints(loss):
    sd = loss.state_dict()
    assert list(sd) == [e["key"] for e in REF["state_dict"]]
    for e in REF["state_dict"]:
        assert list(sd[e["key"]].shape) == e["shape"]
        assert lc.fingerprint(sd[e["key"]].cpu().numpy()) == (e["sum"], e["sum_sq"]), e["key"]


def _cpu_stack(cpu_loss, x):
    """This module's nn.Conv1d stacks run by torch on the CPU in float32."""
    disc = cpu_loss.adversarial_loss.discriminator
    outs, feats = [], []
    with torch.no_grad():
        for s, seq in zip(disc.scales, disc.discriminators):
            h = x if s == 1 else F.avg_pool1d(x, s, s)
            maps = []
            for layer in seq:
                h = layer(h)
                if isinstance(layer, torch.nn.Conv1d) and h.size(1) > 1:
                    maps.append(h)
            outs.append(h)
            feats.append(maps)
    return outs, feats


@pytest.mark.parametrize("case", lc.DISC_CASES)
def test_discriminator_matches_recorded_float64(gpu, loss, cpu_loss, case):
    rec = REF["cases"][case]
    _, target = lc.audio_case(case)
    x = torch.from_numpy(target)
    outs, feats = loss.adversarial_loss.discriminator(x.to(gpu))
    cpu_outs, cpu_feats = _cpu_stack(cpu_loss, x)
    assert len(outs) == 3 and [len(m) for m in feats] == [6, 6, 6]
    assert rec["feature_matching_normaliser"] == 18 == sum(len(m) for m in feats)
    for s in range(3):
        want = torch.from_numpy(REF_ARRAYS[f"{case}.logits{s}"])
        assert list(outs[s].shape) == rec["logit_shapes"][s] and outs[s].dtype == torch.float32 and outs[s].is_cuda
        top = float(want.abs().max())
        sp = float((cpu_outs[s].reshape(-1).double() - want).abs().max()) / top
        err = float((outs[s].cpu().reshape(-1).double() - want).abs().max()) / top
        print(f"{case} scale {s} logits: rel max err {err:.3e}, cpu float32 {sp:.3e}, bar {32 * max(sp, EPS):.3e}")
        assert err <= 32.0 * max(sp, EPS), (case, s)
        for l in range(6):
            r = rec["features"][s][l]
            f = feats[s][l]
            assert list(f.shape) == r["shape"] and not f.requires_grad
            idx = torch.from_numpy(lc.sample_indices(s, l, f.numel()))
            want = torch.from_numpy(REF_ARRAYS[f"{case}.s{s}l{l}"])
            top = r["max_abs"]
            sp = float((cpu_feats[s][l].reshape(-1)[idx].double() - want).abs().max()) / top
            bar = 32.0 * max(sp, EPS)
            flat = f.cpu().reshape(-1).double()
            err = float((flat[idx] - want).abs().max()) / top
            mean_err = abs(float(flat.abs().mean()) - r["mean_abs"]) / top
            print(f"{case} scale {s} layer {l}: samples {err:.3e}, mean|.| {mean_err:.3e}, cpu float32 {sp:.3e}, "
                  f"bar {bar:.3e}")
            assert err <= bar and mean_err <= bar, (case, s, l)
            assert abs(float(flat.abs().max()) - top) <= bar * top, (case, s, l)


@pytest.mark.parametrize("case", lc.DISC_CASES)
def test_adversarial_scalars_match_reference(gpu, loss, case):
    adv = loss.adversarial_loss
    pred, target = (torch.from_numpy(a).to(gpu) for a in lc.audio_case(case))
    want = REF["cases"][case]["adversarial"]["f64"]
    got = {"generator_loss": adv.generator_loss(pred), "feature_matching_loss": adv.feature_matching_loss(target, pred),
           "discriminator_loss": adv.discriminator_loss(target, pred)}
    for k, v in got.items():
        assert v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda and not v.requires_grad
        _check_scalar(float(v), want[k], k, case)
    # the normaliser is the reference's len(real_features) * len(real_features[0]) = 18, and the
    # sums are those of the maps forward() returns
    _, fr = adv.discriminator(target)
    of, ff = adv.discriminator(pred)
    fm = sum(float((a.double() - b.double()).abs().mean()) for ra, fa in zip(fr, ff) for a, b in zip(fa, ra)) / 18
    assert abs(float(got["feature_matching_loss"]) - fm) <= 32 * EPS * fm
    gen = sum(float(((o.double() - 1) ** 2).mean()) for o in of) / 3
    assert abs(float(got["generator_loss"]) - gen) <= 32 * EPS * gen


# ---- CombinedTTSLoss -------------------------------------------------------------

def _stft64(x, n_fft):
    """torch.stft on the CPU in float64: [B, F, T] complex128 numpy."""
    return torch.stft(torch.from_numpy(x).double().squeeze(1), n_fft=n_fft, hop_length=n_fft // 4,
                      window=torch.hann_window(n_fft, dtype=torch.float64), return_complex=True).numpy()


def _take_flips(X64, Xgpu, bar, counts):
    """X64 with, in every bin with re < 0 whose im differs in sign from the GPU's,
    the GPU's sign of im; each such bin must be unresolvable: |im_f64| <= bar."""
    flip = (X64.real < 0) & (np.signbit(X64.imag) != np.signbit(Xgpu.imag))
    assert np.all(np.abs(X64.imag)[flip] <= np.broadcast_to(bar, X64.shape)[flip]), "a resolvable bin changed sign"
    counts[0] += int(flip[:, :, 0].sum())
    counts[1] += int(flip[:, :, 1:].sum())
    counts[2] += int(flip[:, :, -1].sum())
    out = X64.copy()
    out.imag[flip] = np.copysign(np.abs(X64.imag[flip]), Xgpu.imag[flip])
    return out


def _spectral_expectation(gpu, case):
    """The checks (1), (2), (4) of the module docstring per n_fft; returns expectation (3)."""
    from m2amd.dsp import get_dsp, loss_columns
    pred, target = lc.audio_case(case)
    cols = loss_columns("spectral")
    total = 0.0
    for n_fft in lc.N_FFTS:
        d = get_dsp(lc.SR, n_fft, n_fft // 4, n_fft, device=gpu)
        rows, sp, st = d.loss_spectral(torch.from_numpy(pred).to(gpu), torch.from_numpy(target).to(gpu), spectra=True)
        rows = dict(zip(cols, rows.cpu().numpy().T))
        G = [sp.cpu().numpy(), st.cpu().numpy()]
        X = [_stft64(pred, n_fft), _stft64(target, n_fft)]
        counts = [0, 0, 0]  # flips in frame 0, in the other frames, of those in the last frame
        adj = []
        for g, x in zip(G, X):
            assert g.shape == x.shape and g.dtype == np.complex64
            bar = 32 * 2e-6 * np.abs(x).max(axis=(1, 2), keepdims=True)
            err = np.abs(g.astype(np.complex128) - x)
            print(f"{case} n_fft {n_fft}: spectrum max err / max|X| {float((err / bar).max()) * 32 * 2e-6:.3e} "
                  f"(bar {32 * 2e-6:.3e})")
            assert np.all(err <= bar)  # (1)
            assert np.all(g.imag[:, 0] == 0) and np.all(g.imag[:, -1] == 0)
            assert not np.signbit(g.imag[:, 0]).any() and not np.signbit(g.imag[:, -1]).any()
            adj.append(_take_flips(x, g, bar, counts))  # (4)
        g64 = [g.astype(np.complex128) for g in G]
        for b in range(pred.shape[0]):  # (2)
            mag = np.abs(np.abs(g64[0][b]) - np.abs(g64[1][b])).sum()
            ph = np.abs(np.angle(g64[0][b]) - np.angle(g64[1][b])).sum()
            assert abs(rows["mag_abs"][b] - mag) <= 32 * EPS * mag and abs(rows["phase_abs"][b] - ph) <= 32 * EPS * ph
            assert rows["bins"][b] == g64[0][b].size and rows["frames"][b] == g64[0].shape[2]
        last = "symmetric too" if len(lc.symmetric_frames(pred.shape[-1], n_fft // 4)) > 1 else "not symmetric"
        print(f"{case} n_fft {n_fft}: flips in frame 0: {counts[0]}, in other frames: {counts[1]} "
              f"(of {2 * adj[0][:, :, 0].size} and {2 * adj[0][:, :, 1:].size} bins); {counts[2]} of the latter in "
              f"the last frame, which is {last}")
        total += lc.stft_loss(adj[0], adj[1])
    return total / len(lc.N_FFTS)


@pytest.mark.parametrize("case", lc.FULL_CASES)
def test_combined_loss_matches_reference(gpu, loss, case):
    rec = REF["cases"][case]
    kw = _kw(case, gpu)
    step = loss.training_step
    gen = loss(**kw, optimize_discriminator=False)
    dis = loss(**kw, optimize_discriminator=True)
    assert loss.training_step == step + 2
    assert list(gen) == REF["dict_keys"]["generator"] and list(dis) == REF["dict_keys"]["discriminator"]
    for d in (gen, dis):
        for v in d.values():
            assert v.dim() == 0 and v.dtype == torch.float32 and v.device == gpu and not v.requires_grad
    for k in ("mel_loss", "duration_loss", "perceptual_loss", "generator_loss", "feature_matching_loss"):
        _check_scalar(float(gen[k]), rec["generator"]["f64"][k], k, f"{case} generator")
    for k in ("mel_loss", "duration_loss", "perceptual_loss", "discriminator_loss"):
        _check_scalar(float(dis[k]), rec["discriminator"]["f64"][k], k, f"{case} discriminator")
    assert torch.equal(dis["total_loss"], dis["discriminator_loss"])

    want = _spectral_expectation(gpu, case)
    bar = 32.0 * max(rec["spectral_forced"]["spread"], EPS)
    for d in (gen, dis):
        got = float(d["spectral_loss"])
        print(f"{case} spectral_loss: got {got!r}, float64 with the GPU's flips {want!r}, rel "
              f"{abs(got - want) / want:.3e}, bar {bar:.3e}; the reference's float32 {rec['generator']['f32']['spectral_loss']!r}, "
              f"float64 {rec['generator']['f64']['spectral_loss']!r}")
        assert abs(got - want) <= bar * want
    # total = the weighted sum; each term within its own bar, plus the float32 result's rounding
    parts = dict(rec["generator"]["f64"], spectral_loss=want)
    total = sum(w * parts[k] for k, w in WEIGHTS.items())
    tol = sum(w * parts[k] * (bar if k == "spectral_loss" else _bar(k)) for k, w in WEIGHTS.items()) + 32 * EPS * total
    print(f"{case} total_loss: got {float(gen['total_loss'])!r}, expected {total!r}, tolerance {tol:.3e}")
    assert abs(float(gen["total_loss"]) - total) <= tol

    again = loss(**kw, optimize_discriminator=False)  # two runs give equal bits
    assert all(torch.equal(again[k], gen[k]) for k in gen)


def test_no_audio_and_no_discriminator(gpu, loss):
    from training.losses import CombinedTTSLoss
    rec = REF["cases"]["smoke40"]
    kw = _kw("smoke40", gpu)
    audio = {k: kw.pop(k) for k in ("audio_pred", "audio_target")}
    got = loss(**kw)
    assert list(got) == REF["dict_keys"]["no_audio"]
    for k in got:
        _check_scalar(float(got[k]), rec["no_audio"]["f64"][k], k, "smoke40 no audio", modes=("no_audio",))
    assert list(loss(**kw, audio_pred=audio["audio_pred"])) == REF["dict_keys"]["no_audio"]  # both are needed
    # without mel_lengths: the plain mean
    kw2 = dict(kw, mel_lengths=None)
    want = np.abs(lc.loss_case("smoke40")["mel_pred"].astype(np.float64)
                  - lc.loss_case("smoke40")["mel_target"].astype(np.float64).transpose(0, 2, 1)).mean()
    assert abs(float(loss(**kw2)["mel_loss"]) - want) <= 32 * EPS * want
    plain = CombinedTTSLoss(use_discriminator=False)
    assert plain.adversarial_loss is None and plain.get_discriminator_parameters() == []
    out = plain(**kw, **audio)
    assert list(out) == ["mel_loss", "duration_loss", "spectral_loss", "perceptual_loss", "total_loss"]
    assert plain.training_step == 1
    full = loss(**kw, **audio)
    for k in ("mel_loss", "duration_loss", "spectral_loss", "perceptual_loss"):
        assert torch.equal(out[k], full[k])
    assert list(plain(**kw, **audio, optimize_discriminator=True)) == list(out) and plain.training_step == 2


def test_batched_rows_equal_single_rows(gpu, loss):
    from m2amd.dsp import get_dsp, loss_columns
    pred, target = (torch.from_numpy(a).to(gpu) for a in lc.audio_case("odd"))
    h = loss.adversarial_loss.discriminator._handle(gpu)
    rows = h.losses(target, pred)
    assert rows.shape == (3, len(loss_columns("disc"))) and rows.dtype == torch.float64 and rows.is_cuda
    assert torch.equal(rows, h.losses(target, pred))
    for b in range(3):
        assert torch.equal(rows[b:b + 1], h.losses(target[b:b + 1], pred[b:b + 1]))
    c = dict(zip(loss_columns("disc"), rows[0].tolist()))
    lens = [lc.layer_lengths(1001, s) for s in lc.SCALES]
    for s in range(3):
        assert c[f"s{s}_logits"] == lens[s][6]
        for l in range(6):
            assert c[f"s{s}_l{l}_count"] == lc.LAYERS[l][1] * lens[s][l]
    only_fake = dict(zip(loss_columns("disc"), h.losses(None, pred)[0].tolist()))
    assert only_fake["s1_fake_err_sq"] == c["s1_fake_err_sq"] and only_fake["s1_real_sq"] == 0.0
    assert only_fake["s2_l3_abs_diff"] == 0.0
    pred, target = (torch.from_numpy(a).to(gpu).squeeze(1) for a in lc.audio_case("edge41"))
    for n_fft in lc.N_FFTS:
        d = get_dsp(lc.SR, n_fft, n_fft // 4, n_fft, device=gpu)
        w = torch.linspace(0, 1, 80, device=gpu)
        rows = d.loss_spectral(pred, target, w)
        assert torch.equal(rows, d.loss_spectral(pred, target, w))
        for b in range(2):
            assert torch.equal(rows[b:b + 1], d.loss_spectral(pred[b:b + 1], target[b:b + 1], w))
        assert bool((d.loss_spectral(pred, target)[:, 3] == 0).all())  # no weights: no perceptual sum


def test_load_state_dict_rebuilds_the_packed_weights(gpu):
    from training.losses import MultiScaleDiscriminator
    torch.manual_seed(7)
    a = MultiScaleDiscriminator().to(gpu)
    x = torch.from_numpy(lc.audio_case("odd")[1]).to(gpu)
    before = [o.clone() for o in a(x)[0]]
    sd = {k: v + 0.01 * torch.randn_like(v) for k, v in a.state_dict().items()}
    a.load_state_dict(sd)
    after = a(x)[0]
    assert all(not torch.equal(p, q) for p, q in zip(before, after))
    b = MultiScaleDiscriminator()
    b.load_state_dict(sd)
    assert all(torch.equal(p, q) for p, q in zip(after, b.to(gpu)(x)[0]))
    with torch.no_grad():
        next(a.parameters()).mul_(2.0)  # an in-place update, as an optimizer step makes
    assert not torch.equal(a(x)[0][0], after[0])


def test_packed_layers_chain_to_the_forward(gpu, loss):
    """forward() is the seven packed layers in a row (m2_disc_layer), pooled audio in: equal bits,
    with and without the feature buffer, and through the sliced losses call."""
    from m2amd import ops
    from m2amd.dsp import loss_columns
    x = torch.from_numpy(lc.audio_case("odd")[1]).to(gpu)
    h = loss.adversarial_loss.discriminator._handle(gpu)
    outs, feats = h.forward(x)
    bare, none = h.forward(x, features=False)
    assert none is None and all(torch.equal(a, b) for a, b in zip(outs, bare))
    c = dict(zip(loss_columns("disc"), h.losses(x, None).sum(0).tolist()))
    for s, scale in enumerate(lc.SCALES):
        y = x if scale == 1 else ops.avg_pool1d(x, scale)
        for layer in range(7):
            y = h.layer(s, layer, y)
            assert torch.equal(y, feats[s][layer] if layer < 6 else outs[s]), (s, layer)
        want = float((outs[s].double() ** 2).sum())
        assert abs(c[f"s{s}_real_sq"] - want) <= 1e-12 * want


def test_batch_slices_give_the_same_bits(gpu):
    """A slice bound that admits two utterances (one in the losses call, which holds real and fake)
    walks the batch of three in two (three) slices: same logits, maps and rows."""
    from training.losses import MultiScaleDiscriminator
    torch.manual_seed(3)
    disc = MultiScaleDiscriminator().to(gpu)
    pred, target = (torch.from_numpy(a).to(gpu) for a in lc.audio_case("odd"))
    h = disc._handle(gpu)
    outs, feats = h.forward(target)
    bare, _ = h.forward(target, features=False)
    rows = h.losses(target, pred)
    per_utterance = 4 * sum(-(-c * n // 64) * 64 for c, n in h.shapes(1001)[0])
    h.set_slice_bytes(2 * per_utterance + 4)
    outs2, feats2 = h.forward(target)
    bare2, _ = h.forward(target, features=False)
    assert all(torch.equal(a, b) for a, b in zip(outs + bare, outs2 + bare2))
    assert all(torch.equal(a, b) for fa, fb in zip(feats, feats2) for a, b in zip(fa, fb))
    assert torch.equal(rows, h.losses(target, pred))
    h.set_slice_bytes(0)
    assert torch.equal(rows, h.losses(target, pred))


def test_errors(gpu, loss):
    pred, target = (torch.from_numpy(a).to(gpu) for a in lc.audio_case("one"))
    with pytest.raises(RuntimeError):
        loss.spectral_loss(pred[:, :, :1024], target[:, :, :1024])  # reflect padding of 2048 needs 1025 samples
    with pytest.raises(RuntimeError):
        loss.spectral_loss(pred, target[:, :, :1024])
    kw = _kw("one", gpu)
    kw["audio_target"] = kw["audio_target"][:, :, :1024]
    step = loss.training_step
    with pytest.raises(RuntimeError):
        loss(**kw)
    assert loss.training_step == step
    assert float(loss.spectral_loss.stft_loss(pred[:, :, :600], target[:, :, :600], 512)) > 0  # 600 > 256
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        loss(**{k: (None if v is None else v.cpu()) for k, v in _kw("one", gpu).items()})


def test_abi_conventions(gpu, loss):
    from m2amd import _lib
    from m2amd.dsp import get_dsp
    lib = _lib.load()
    d = get_dsp(lc.SR, 1024, 256, 1024, device=gpu)
    h = loss.adversarial_loss.discriminator._handle(gpu).handle
    x = torch.zeros(2, 3000, device=gpu)
    out = torch.full((2, 64), -1.0, device=gpu, dtype=torch.float64)
    need = lib.m2_loss_spectral_workspace_bytes(d.handle, 2, 3000)
    ws = torch.empty(max(need, lib.m2_disc_losses_workspace_bytes(h, 2, 3000)), dtype=torch.uint8, device=gpu)
    spec = (x.data_ptr(), x.data_ptr(), 2, 3000, None, 0, out.data_ptr(), None, None, ws.data_ptr())
    assert lib.m2_loss_spectral(d.handle, *spec, 64, None) == -3  # M2_E_WORKSPACE
    assert b"workspace" in lib.m2_last_error()
    assert lib.m2_loss_spectral(None, *spec, need, None) == -1
    assert lib.m2_loss_spectral(d.handle, x.data_ptr(), None, 2, 3000, None, 0, out.data_ptr(), None, None,
                                ws.data_ptr(), need, None) == -1
    assert lib.m2_loss_spectral(d.handle, x.data_ptr(), x.data_ptr(), 2, 512, None, 0, out.data_ptr(), None, None,
                                ws.data_ptr(), need, None) == -2  # M2_E_SHAPE: L <= n_fft / 2
    assert lib.m2_loss_spectral(d.handle, x.data_ptr(), x.data_ptr(), 0, 3000, None, 0, out.data_ptr(), None, None,
                                None, 0, None) == 0
    assert lib.m2_loss_spectral_workspace_bytes(None, 2, 3000) == 0
    disc = (x.data_ptr(), x.data_ptr(), 2, 3000, out.data_ptr(), ws.data_ptr())
    assert lib.m2_disc_losses(h, *disc, 64, None) == -3
    assert lib.m2_disc_losses(None, *disc, ws.numel(), None) == -1
    assert lib.m2_disc_losses(h, None, None, 2, 3000, out.data_ptr(), ws.data_ptr(), ws.numel(), None) == -1
    assert lib.m2_disc_losses(h, x.data_ptr(), None, 0, 3000, out.data_ptr(), None, 0, None) == 0
    assert lib.m2_disc_losses(h, x.data_ptr(), None, 2, 3, out.data_ptr(), ws.data_ptr(), ws.numel(), None) == -2
    assert lib.m2_disc_forward(h, x.data_ptr(), 2, 3000, out.data_ptr(), None, ws.data_ptr(), 64, None) == -3
    assert lib.m2_disc_forward(h, x.data_ptr(), 0, 3000, out.data_ptr(), None, None, 0, None) == 0
    assert lib.m2_disc_forward_workspace_bytes(None, 2, 3000) == 0 == lib.m2_disc_losses_workspace_bytes(None, 2, 3000)
    conv = (x.data_ptr(), x.data_ptr(), None)
    assert lib.m2_conv1d_strided(*conv, 3, 1, 1, 4, 1.0, 2, 6, 6, 100, out.data_ptr(), None) == -2  # groups 4, 6 channels
    assert lib.m2_conv1d_strided(*conv, 3, 0, 1, 1, 1.0, 2, 6, 6, 100, out.data_ptr(), None) == -1  # stride 0
    assert lib.m2_conv1d_strided(*conv, 9, 1, 1, 1, 1.0, 2, 6, 6, 4, out.data_ptr(), None) == -2  # k > L + 2 p
    assert lib.m2_conv1d_strided(*conv, 3, 1, 1, 1, 1.0, 0, 6, 6, 100, out.data_ptr(), None) == 0
    assert lib.m2_avg_pool1d(None, 2, 2, 1, 100, out.data_ptr(), None) == -1
    assert lib.m2_disc_create(None, 42, None, 3, None, None) == -1
    assert lib.m2_loss_column_count(2) == -1 and lib.m2_loss_column_name(0, 99) is None
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())  # nothing was launched
