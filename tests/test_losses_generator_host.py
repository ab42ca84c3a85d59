"""Host-side checks of the generator step's gradient (no GPU): the new entry
points are exported and bound with the header's signatures, bad arguments are
reported, CPU tensors are refused with the switch on and a prediction that
requires grad, and the masked float64 oracle the GPU tests compare against
equals plain torch autograd of the reference's formulas when its masks and
signs come from itself."""
import ctypes
import sys

import pytest
import torch

import test_ragged_host
from conftest import GOLDEN

sys.path.insert(0, str(GOLDEN))
import losses_backward_oracle as orc  # noqa: E402
import losses_cases as lc  # noqa: E402
import losses_generator_oracle as gorc  # noqa: E402

ENTRIES = {"m2_disc_gen_step_workspace_bytes": 3, "m2_disc_gen_step": 12, "m2_conv1d_audio_backward": 11}


@pytest.fixture(scope="module")
def seeded():
    from training.losses import CombinedTTSLoss
    torch.manual_seed(lc.WEIGHT_SEED)
    return CombinedTTSLoss().eval()


@pytest.mark.parametrize("name", ENTRIES)
def test_entry_points_exported_and_bound(name, monkeypatch):
    from m2amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name), f"{name} is not exported by the library"
    monkeypatch.setitem(test_ragged_host.CTYPES, "double", ctypes.c_double)  # the weights of m2_disc_gen_step
    res, args = test_ragged_host.header_signature(name)
    assert _lib._SIGNATURES[name] == (res, args)
    assert len(args) == ENTRIES[name]
    fn = getattr(lib, name)
    assert fn.restype is res and list(fn.argtypes) == args
    assert name in _lib.exported_symbols()


def test_bad_arguments_are_reported():
    from m2amd import _lib
    lib = _lib.load()
    assert lib.m2_disc_gen_step(None, None, None, 1, 1, 1.0, 0.0, None, None, None, 0, None) == -1
    assert b"m2_disc_gen_step" in lib.m2_last_error()
    assert lib.m2_conv1d_audio_backward(None, None, 15, 7, 1, 1, 64, 100, 0, None, None) == -1
    assert b"m2_conv1d_audio_backward" in lib.m2_last_error()
    buf = (ctypes.c_float * 4)()
    p = ctypes.addressof(buf)
    for bad in ((0, 7, 1, 1, 64, 100), (15, -1, 1, 1, 64, 100), (15, 7, 0, 1, 64, 100), (15, 7, 1, -1, 64, 100),
                (15, 7, 1, 1, 0, 100), (15, 7, 1, 1, 64, 0)):
        assert lib.m2_conv1d_audio_backward(p, p, *bad, 0, p, None) == -1, bad
    # shapes the kernel cannot take: a window beyond LDS, pooled input shorter than the kernel allows
    assert lib.m2_conv1d_audio_backward(p, p, 15, 7, 1, 1, 4096, 100, 0, p, None) == -2
    assert lib.m2_conv1d_audio_backward(p, p, 15, 0, 4, 1, 64, 40, 0, p, None) == -2  # 10 pooled samples, k = 15
    assert lib.m2_conv1d_audio_backward(p, p, 15, 7, 4, 1, 64, 3, 0, p, None) == -2   # no pooled sample
    assert b"m2_conv1d_audio_backward" in lib.m2_last_error()
    assert lib.m2_conv1d_audio_backward(p, p, 15, 7, 1, 0, 64, 100, 0, p, None) == 0  # B == 0
    assert lib.m2_disc_gen_step_workspace_bytes(None, 2, 3000) == 0


def test_cpu_tensors_raise_with_the_switch_on(seeded):
    kw = {k: (None if v is None else torch.from_numpy(v)) for k, v in lc.loss_case("one").items()}
    adv = seeded.adversarial_loss
    seeded.enable_backward()
    try:
        for k in ("audio_pred", "mel_pred", "duration_pred"):
            kw[k].requires_grad_(True)
        assert torch.is_grad_enabled()
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            seeded(**kw)
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            adv.generator_loss(kw["audio_pred"])
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            adv.feature_matching_loss(kw["audio_target"], kw["audio_pred"])
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            adv.generator_terms(kw["audio_target"], kw["audio_pred"], 0.25, 2.0)
        assert seeded.training_step == 0
    finally:
        seeded.enable_backward(False)
    assert seeded.backward_enabled is False and type(seeded).backward_enabled is False
    assert len(seeded.state_dict()) == 42


def test_attach_gradients_on_the_cpu():
    """The autograd plumbing itself needs no GPU: value unchanged, grad_output * g cast and reshaped."""
    from training.losses import _attach
    x = torch.arange(6.0, dtype=torch.float64).reshape(2, 3).requires_grad_()
    y = torch.ones(3, requires_grad=True)
    v = torch.tensor(1.25)
    out = _attach(v, [(x, torch.arange(6.0)), (y, torch.full((1, 3), 2.0))])
    assert torch.equal(out.detach(), v) and out.grad_fn is not None and v.grad_fn is None
    (3.0 * out).backward()
    assert x.grad.dtype == torch.float64 and torch.equal(x.grad, 3.0 * torch.arange(6.0, dtype=torch.float64).reshape(2, 3))
    assert torch.equal(y.grad, torch.full((3,), 6.0))
    with pytest.raises(RuntimeError):
        (g,) = torch.autograd.grad(_attach(v, [(x, torch.arange(6.0))]), x, create_graph=True)
        g.sum().backward()


@pytest.mark.parametrize("weights", [(1.0, 0.0), (0.0, 1.0), (0.25, 2.0)])
def test_masked_oracle_equals_plain_autograd_with_its_own_masks_and_signs(seeded, weights):
    disc = seeded.adversarial_loss.discriminator
    stacks = orc.cpu_stacks(disc, torch.float64)
    fake, real = (torch.from_numpy(a).double() for a in lc.audio_case("one"))
    w_adv, w_fm = weights
    r = real if w_fm else None
    value, g, rm, fm = gorc.gradient(stacks, disc.scales, r, fake, w_adv, w_fm)
    value2, plain = gorc.plain_gradient(stacks, disc.scales, r, fake, w_adv, w_fm)
    assert g.shape == fake.shape and float(plain.abs().max()) > 0
    assert abs(float(value) - float(value2)) <= 1e-14 * abs(float(value2))
    assert float((g - plain).abs().max()) <= 1e-12 * float(plain.abs().max())
    if not w_fm:
        assert rm is None
        return
    # masks and signs given explicitly reproduce it bit for bit; a flipped sign changes the result
    pos_r, pos_f, sg = gorc.masks(rm), gorc.masks(fm), gorc.signs_of(fm, rm, torch.float64)
    _, again, _, _ = gorc.gradient(stacks, disc.scales, real, fake, w_adv, w_fm, pos_r, pos_f, sg)
    assert float((again - g).abs().max()) <= 1e-12 * float(g.abs().max())
    sg[0][0] = -sg[0][0]
    _, flipped, _, _ = gorc.gradient(stacks, disc.scales, real, fake, w_adv, w_fm, pos_r, pos_f, sg)
    assert float((flipped - g).abs().max()) > 1e-6 * float(g.abs().max())
    assert all(p.grad is None for p in orc.parameters(stacks))
