"""Host-side checks of the gradient of the spectral and perceptual losses (no GPU): the oracle
the GPU tests compare against (tests/golden/losses_spectral_oracle.py) equals float64 autograd of
the formula over torch.stft, its conventions at |P| = 0 and at equal signals hold, the coefficient
helper of training.losses gives the means' reciprocals, the new entry points are exported and bound
with the header's signatures and report bad arguments, and the switches default to off."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import test_ragged_host
from conftest import GOLDEN

sys.path.insert(0, str(GOLDEN))
import losses_cases as lc  # noqa: E402
import losses_spectral_oracle as sorc  # noqa: E402

ENTRIES = {"m2_loss_spectral_backward_workspace_bytes": 3, "m2_loss_spectral_backward": 16}
CASES = ("one", "edge41", "smoke40")


def _pair(case):
    pred, target = lc.audio_case(case)
    return torch.from_numpy(pred[:, 0]).double(), torch.from_numpy(target[:, 0]).double()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("n_fft", lc.N_FFTS)
def test_closed_form_equals_float64_autograd(case, n_fft):
    """cotangent + adjoint against autograd of the plain formula, all three terms at once with the
    losses' coefficients; `one` at n_fft 2048 is where both reflections overlap."""
    pred, target = _pair(case)
    B, L = pred.shape
    hop = n_fft // 4
    w = sorc.mel_weights(n_fft // 2 + 1).numpy()
    c = sorc.coefficients(B, L, n_fft, hop)
    want = sorc.gradient(pred, target, n_fft, hop, w, *c).numpy()
    P, T = sorc.stft(pred, n_fft, hop).numpy(), sorc.stft(target, n_fft, hop).numpy()
    got = sorc.adjoint(sorc.cotangent(P, T, w, *c), n_fft, hop, L)
    top = np.abs(want).max()
    err = np.abs(got - want).max()
    print(f"{case} n_fft {n_fft}: max|g| {top:.3e}, closed form - autograd {err:.3e}")
    assert top > 0 and err <= 1e-12 * top
    # each term alone, and the signs prescribed from the spectra themselves change nothing
    signs = sorc.signs_of(P, T, w)
    for k in range(3):
        ck = [c[j] if j == k else 0.0 for j in range(3)]
        want = sorc.gradient(pred, target, n_fft, hop, w, *ck).numpy()
        got = sorc.adjoint(sorc.cotangent(P, T, w, *ck), n_fft, hop, L)
        imposed = sorc.gradient(pred, target, n_fft, hop, w, *ck, signs=signs).numpy()
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), k
        assert np.abs(imposed - want).max() <= 1e-12 * np.abs(want).max(), k


def test_a_hop_that_does_not_divide_n_fft():
    g = torch.Generator().manual_seed(777)
    pred, target = torch.randn(2, 777, generator=g).double(), torch.randn(2, 777, generator=g).double()
    w = sorc.mel_weights(257).numpy()
    c = sorc.coefficients(2, 777, 512, 200)
    want = sorc.gradient(pred, target, 512, 200, w, *c).numpy()
    P, T = sorc.stft(pred, 512, 200).numpy(), sorc.stft(target, 512, 200).numpy()
    got = sorc.adjoint(sorc.cotangent(P, T, w, *c), 512, 200, 777)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_flipped_sign_changes_the_gradient():
    pred, target = _pair("one")
    w = sorc.mel_weights(257).numpy()
    P, T = sorc.stft(pred, 512, 128).numpy(), sorc.stft(target, 512, 128).numpy()
    sm, sa, sp = sorc.signs_of(P, T, w)
    assert sp[:, 0].tolist() == np.zeros_like(sp[:, 0]).tolist()  # w_0 = 0 contributes nothing
    assert set(np.unique(sm)) <= {-1.0, 0.0, 1.0} and np.abs(sp[:, 1:]).min() == 1.0
    base = sorc.gradient(pred, target, 512, 128, w, 0.0, 1.0, 0.0, signs=(sm, sa, sp)).numpy()
    sa = sa.copy()
    sa[0, 5, 3] = -sa[0, 5, 3]
    flipped = sorc.gradient(pred, target, 512, 128, w, 0.0, 1.0, 0.0, signs=(sm, sa, sp)).numpy()
    assert np.abs(flipped - base).max() > 1e-6 * np.abs(base).max()
    g = sorc.cotangent(P, T, w, 0.0, 1.0, 0.0, signs=(sm, sa, sp))
    assert np.abs(sorc.adjoint(g, 512, 128, pred.shape[1]) - flipped).max() <= 1e-12 * np.abs(flipped).max()


def test_zero_and_equal_conventions():
    pred, target = _pair("one")
    B, L = pred.shape
    w = sorc.mel_weights(257).numpy()
    c = sorc.coefficients(B, L, 512, 128)
    T = sorc.stft(target, 512, 128).numpy()
    # pred == target: every sign is 0, so is the cotangent; autograd agrees (abs'(0) = 0)
    assert not sorc.cotangent(T, T, w, *c).any()
    assert not sorc.gradient(target, target, 512, 128, w, *c).numpy().any()
    # pred == 0: |P| = 0 everywhere, finite zeros from both
    zero = torch.zeros_like(pred)
    g = sorc.cotangent(np.zeros_like(T), T, w, *c)
    assert np.isfinite(g).all() and not g.any()
    auto = sorc.gradient(zero, target, 512, 128, w, *c).numpy()
    assert np.isfinite(auto).all() and not auto.any()
    assert not sorc.adjoint(g, 512, 128, L).any()


def test_coefficient_helper():
    from training.losses import spectral_backward_calls
    B, L = 32, 32000
    calls = spectral_backward_calls(B, L, [512, 1024, 2048], 0.25, 1.0, 0.5)
    assert [c[:2] for c in calls] == [(512, 128), (1024, 256), (2048, 512)]
    for n_fft, hop, c_mag, c_ph, c_perc in calls:
        frames = 1 + L // hop
        assert c_mag == pytest.approx(1.0 / (3 * B * (n_fft // 2 + 1) * frames), rel=1e-15)
        assert c_ph == pytest.approx(0.1 * c_mag, rel=1e-15)
        assert c_perc == pytest.approx(0.5 / (B * 80 * frames) if n_fft == 1024 else 0.0, rel=1e-15)
        want = sorc.coefficients(B, L, n_fft, hop)
        assert (c_mag, c_ph) == pytest.approx(want[:2], rel=1e-15)
    # a term of weight 0 makes no call; the perceptual term alone is one call at 1024 / 256
    assert spectral_backward_calls(B, L, [512, 1024, 2048], 0.25, 0.0, 0.0) == []
    (only,) = spectral_backward_calls(2, 2560, [512, 1024, 2048], 0.25, 0.0, 1.0)
    assert only == (1024, 256, 0.0, 0.0, pytest.approx(1.0 / (2 * 80 * 11)))
    assert [c[:2] for c in spectral_backward_calls(2, 2560, [512], 0.25, 2.0, 1.0)] == [(512, 128), (1024, 256)]
    assert spectral_backward_calls(0, 2560) == []


@pytest.mark.parametrize("name", ENTRIES)
def test_entry_points_exported_and_bound(name, monkeypatch):
    from m2amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name), f"{name} is not exported by the library"
    monkeypatch.setitem(test_ragged_host.CTYPES, "double", ctypes.c_double)  # the three coefficients
    res, args = test_ragged_host.header_signature(name)
    assert _lib._SIGNATURES[name] == (res, args)
    assert len(args) == ENTRIES[name]
    fn = getattr(lib, name)
    assert fn.restype is res and list(fn.argtypes) == args
    assert name in _lib.exported_symbols()


def test_bad_arguments_are_reported():
    from m2amd import _lib
    lib = _lib.load()
    assert lib.m2_loss_spectral_backward(None, None, None, 1, 1000, None, 0, 1.0, 0.1, 0.0, 0, None, None, None, 0,
                                         None) == -1
    assert b"m2_loss_spectral_backward" in lib.m2_last_error()
    assert lib.m2_loss_spectral_backward_workspace_bytes(None, 2, 3000) == 0


def test_switches_default_off_and_stay_out_of_the_state_dict():
    from training.losses import CombinedTTSLoss, PerceptualLoss, SpectralLoss
    m = CombinedTTSLoss()
    subs = (m.spectral_loss, m.perceptual_loss)
    assert not any(s.backward_enabled for s in subs)
    assert m.enable_backward() is m and m.backward_enabled and not any(s.backward_enabled for s in subs)
    m.enable_backward(spectral=True)
    assert m.backward_enabled and all(s.backward_enabled for s in subs)
    m.enable_backward(False, spectral=True)
    assert not m.backward_enabled and not any(s.backward_enabled for s in subs)
    m.enable_backward(spectral=True)
    m.enable_backward()  # a plain call switches the spectral gradient off again
    assert m.backward_enabled and not any(s.backward_enabled for s in subs)
    m.enable_backward(False)
    assert len(m.state_dict()) == 42
    assert SpectralLoss.backward_enabled is False and PerceptualLoss.backward_enabled is False
    s = SpectralLoss()
    assert s.enable_backward() is s and s.backward_enabled and not SpectralLoss().backward_enabled
    assert len(s.state_dict()) == 0


def test_cpu_tensors_raise_with_the_switch_on():
    from training.losses import PerceptualLoss, SpectralLoss
    pred, target = (torch.from_numpy(a) for a in lc.audio_case("one"))
    pred.requires_grad_(True)
    for module in (SpectralLoss().enable_backward(), PerceptualLoss().enable_backward()):
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            module(pred, target)
