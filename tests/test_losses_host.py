"""Host-side checks of the drop-in training.losses module (no GPU): it imports
and constructs anywhere, its state_dict is the reference's (keys, order,
shapes, seeded values), EarlyStopping answers like the reference's, and CPU
tensors are refused.  Expected values: tests/golden/losses_reference.json,
recorded from the reference by tests/golden/make_losses_golden.py."""
import json
import sys

import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, str(GOLDEN))
import losses_cases as lc  # noqa: E402

REF = json.loads((GOLDEN / "losses_reference.json").read_text())


@pytest.fixture(scope="module")
def seeded():
    from training.losses import CombinedTTSLoss
    torch.manual_seed(lc.WEIGHT_SEED)
    return CombinedTTSLoss().eval()


def test_module_surface(seeded):
    from training import losses
    for name in ("SpectralLoss", "MultiScaleDiscriminator", "AdversarialLoss", "PerceptualLoss", "CombinedTTSLoss",
                 "EarlyStopping"):
        assert callable(getattr(losses, name)), name
    assert isinstance(seeded.spectral_loss, losses.SpectralLoss)
    assert isinstance(seeded.perceptual_loss, losses.PerceptualLoss)
    assert len(seeded.adversarial_loss.discriminator.discriminators) == 3
    assert seeded.training_step == 0
    assert seeded.spectral_loss.n_fft_list == [512, 1024, 2048] and seeded.spectral_loss.hop_length_factor == 0.25
    assert (seeded.mel_loss_weight, seeded.duration_loss_weight, seeded.adversarial_loss_weight,
            seeded.feature_matching_weight, seeded.spectral_loss_weight, seeded.perceptual_loss_weight) == \
        (1.0, 0.1, 0.25, 2.0, 1.0, 0.5)
    params = list(seeded.get_discriminator_parameters())
    assert len(params) == 42 and sum(p.numel() for p in params) == 16757379
    plain = losses.CombinedTTSLoss(use_discriminator=False)
    assert plain.adversarial_loss is None and plain.get_discriminator_parameters() == []
    assert len(plain.state_dict()) == 0


def test_state_dict_is_the_references(seeded):
    sd = seeded.state_dict()
    assert [k for k in sd] == [e["key"] for e in REF["state_dict"]]
    assert len(sd) == 42
    for e in REF["state_dict"]:
        assert list(sd[e["key"]].shape) == e["shape"], e["key"]
    # the layer table the GPU tests restate
    for i, (cin, cout, k, _, _, groups) in enumerate(lc.LAYERS):
        assert list(sd[f"adversarial_loss.discriminator.discriminators.0.{2 * i}.weight"].shape) == \
            [cout, cin // groups, k]


def test_seeded_weights_match_the_recorded_fingerprints(seeded):
    sd = seeded.state_dict()
    for e in REF["state_dict"]:
        assert lc.fingerprint(sd[e["key"]].numpy()) == (e["sum"], e["sum_sq"]), e["key"]


def test_early_stopping_matches_reference():
    from training.losses import EarlyStopping
    d, want = EarlyStopping(), REF["early_stopping"]["defaults"]
    assert {"patience": d.patience, "min_delta": d.min_delta, "best_loss": d.best_loss, "wait": d.wait} == want
    es = lc.EARLY_STOPPING
    stopper = EarlyStopping(patience=es["patience"], min_delta=es["min_delta"])
    for x, step in zip(es["sequence"], REF["early_stopping"]["trace"]):
        stop = stopper(x)
        assert {"stop": stop, "best_loss": stopper.best_loss, "wait": stopper.wait} == step, x
    assert any(step["stop"] for step in REF["early_stopping"]["trace"])


def test_cpu_tensors_raise(seeded):
    kw = {k: (None if v is None else torch.from_numpy(v)) for k, v in lc.loss_case("one").items()}
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        seeded(**kw)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        seeded.adversarial_loss.discriminator(kw["audio_pred"])
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        seeded.spectral_loss(kw["audio_pred"], kw["audio_target"])
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        seeded.perceptual_loss(kw["audio_pred"], kw["audio_target"])
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        seeded.adversarial_loss.generator_loss(kw["audio_pred"])
    assert seeded.training_step == 0


def test_case_lengths_are_the_documented_ones():
    assert [lc.layer_lengths(2560, s)[:5] for s in lc.SCALES] == \
        [[2560, 640, 160, 40, 10], [1280, 320, 80, 20, 5], [640, 160, 40, 10, 3]]
    assert [lc.layer_lengths(2624, s)[4] * 2 for s in lc.SCALES] == [22, 12, 6]  # dense-layer columns at B = 2
    assert lc.layer_lengths(1001, 2)[0] == 500 and lc.layer_lengths(1001, 4)[0] == 250
