"""Host-side checks of the discriminator step's backward (no GPU): the switch
is off by default and is no state_dict entry, CPU tensors are refused with it
on, the new entry points are exported and bound with the header's signatures,
and the masked float64 oracle the GPU tests compare against equals plain torch
autograd when its masks come from itself."""
import sys

import pytest
import torch

from conftest import GOLDEN
from test_ragged_host import header_signature

sys.path.insert(0, str(GOLDEN))
import losses_backward_oracle as orc  # noqa: E402
import losses_cases as lc  # noqa: E402

ENTRIES = ["m2_conv1d_strided_backward_workspace_bytes", "m2_conv1d_strided_backward", "m2_disc_step_workspace_bytes",
           "m2_disc_step"]


@pytest.fixture(scope="module")
def seeded():
    from training.losses import CombinedTTSLoss
    torch.manual_seed(lc.WEIGHT_SEED)
    return CombinedTTSLoss().eval()


def test_switch_defaults_to_off_and_is_no_state(seeded):
    from training.losses import AdversarialLoss, CombinedTTSLoss, MultiScaleDiscriminator
    disc = seeded.adversarial_loss.discriminator
    assert disc.backward_enabled is False and MultiScaleDiscriminator().backward_enabled is False
    keys = list(seeded.state_dict())
    assert seeded.enable_backward() is seeded and disc.backward_enabled is True
    assert list(seeded.state_dict()) == keys and len(keys) == 42
    assert not any("backward" in k for k in keys)
    assert "backward_enabled" not in dict(disc.named_buffers()) and "backward_enabled" not in dict(disc.named_parameters())
    seeded.enable_backward(False)
    assert disc.backward_enabled is False
    adv = AdversarialLoss()
    assert adv.enable_backward() is adv and adv.discriminator.backward_enabled is True
    adv.enable_backward(enabled=False)
    assert adv.discriminator.backward_enabled is False
    plain = CombinedTTSLoss(use_discriminator=False)
    assert plain.enable_backward() is plain  # nothing to switch
    # the switch follows the instance, not the class
    assert MultiScaleDiscriminator.backward_enabled is False


def test_cpu_tensors_raise_with_the_switch_on(seeded):
    kw = {k: (None if v is None else torch.from_numpy(v)) for k, v in lc.loss_case("one").items()}
    seeded.enable_backward()
    try:
        assert all(p.requires_grad for p in seeded.get_discriminator_parameters()) and torch.is_grad_enabled()
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            seeded(**kw, optimize_discriminator=True)
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            seeded.adversarial_loss.discriminator_loss(kw["audio_target"], kw["audio_pred"])
        assert seeded.training_step == 0
    finally:
        seeded.enable_backward(False)


@pytest.mark.parametrize("name", ENTRIES)
def test_entry_points_exported_and_bound(name):
    from m2amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name), f"{name} is not exported by the library"
    res, args = header_signature(name)
    assert _lib._SIGNATURES[name] == (res, args)
    assert len(args) == {"m2_conv1d_strided_backward_workspace_bytes": 8, "m2_conv1d_strided_backward": 18,
                         "m2_disc_step_workspace_bytes": 3, "m2_disc_step": 10}[name]
    fn = getattr(lib, name)
    assert fn.restype is res and list(fn.argtypes) == args


def test_bad_arguments_are_reported():
    from m2amd import _lib
    lib = _lib.load()
    assert lib.m2_disc_step(None, None, None, 1, 1, None, None, None, 0, None) == -1
    assert b"m2_disc_step" in lib.m2_last_error()
    assert lib.m2_conv1d_strided_backward(None, None, None, 3, 1, 1, 1, 0.2, 1, 4, 4, 8, None, None, None, None, 0,
                                          None) == -1
    assert b"m2_conv1d_strided_backward" in lib.m2_last_error()
    assert lib.m2_disc_step_workspace_bytes(None, 2, 3000) == 0
    assert lib.m2_conv1d_strided_backward_workspace_bytes(3, 1, 1, 4, 2, 6, 6, 100) == 0  # groups 4, 6 channels
    # the split-K partials: one copy of dw per split, at most 64 splits
    n = lib.m2_conv1d_strided_backward_workspace_bytes(41, 4, 20, 4, 3, 64, 128, 2624)
    assert 128 * 16 * 41 * 4 <= n <= 64 * 128 * 16 * 41 * 4 + 256
    assert lib.m2_conv1d_strided_backward_workspace_bytes(4, 3, 2, 2, 3, 6, 10, 50) == 256  # one workgroup per element


def test_masked_oracle_equals_plain_autograd_with_its_own_masks(seeded):
    """With the masks taken from the stack's own pre-activations the masked product is
    F.leaky_relu: same loss, and the same gradients to float64 rounding."""
    disc = seeded.adversarial_loss.discriminator
    stacks = orc.cpu_stacks(disc, torch.float64)
    assert len(orc.parameters(stacks)) == 42
    assert [tuple(p.shape) for p in orc.parameters(stacks)] == [tuple(v.shape) for v in disc.state_dict().values()]
    fake, real = (torch.from_numpy(a).double() for a in lc.audio_case("one"))
    loss, grads, rm, fm = orc.gradients(stacks, disc.scales, real, fake)
    loss2, plain = orc.plain_gradients(stacks, disc.scales, real, fake)
    assert abs(float(loss) - float(loss2)) <= 1e-14 * abs(float(loss2))
    for g, p in zip(grads, plain):
        assert float((g - p).abs().max()) <= 1e-12 * float(p.abs().max())
    assert [len(m) for m in rm] == [6, 6, 6] == [len(m) for m in fm]
    assert [m.shape[-1] for m in rm[1]] == lc.layer_lengths(1025, 2)[:6]
    # masks given explicitly reproduce it bit for bit, and a flipped mask element changes the result
    pos_r = [[m > 0 for m in row] for row in rm]
    pos_f = [[m > 0 for m in row] for row in fm]
    _, again, _, _ = orc.gradients(stacks, disc.scales, real, fake, pos_r, pos_f)
    assert all(torch.equal(a, b) for a, b in zip(again, grads))
    pos_r[0][5] = ~pos_r[0][5]
    _, flipped, _, _ = orc.gradients(stacks, disc.scales, real, fake, pos_r, pos_f)
    assert not torch.equal(flipped[0], grads[0])
    assert all(p.grad is None for p in orc.parameters(stacks))
