"""GPU: the stage1 vocoder's head and mid stages in one launch (headmid_kernel,
vocoder_x3.hip; M2_HEADMID, default 1) against the three launches
(M2_HEADMID=0): every output keeps its operation sequence, so the audio is
equal bit for bit.  Lengths: one window holding both utterance edges (T = 1,
2, 3), a strip of 250 columns plus its two neighbours at and across the 252
valid positions of a window (61, 62, 63, 64), exactly two full strips (125),
a ragged last strip (126, 137).  The library counts its fused launches
(m2_debug_headmid_launches), so each case also checks the path it took.
"""
import ctypes

import pytest
import torch

import m2tts_oracle as orc
from conftest import AUDIO_RMS_TOL, golden_state, rms, stage_config

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(gpu):
    from models.tts_model import M2TTSModel
    m = M2TTSModel(**stage_config("s1").as_dict())
    m.load_state_dict(golden_state("s1"))
    return m.to(gpu).eval()


def fused_launches():
    from m2amd import _lib
    f = _lib.load().m2_debug_headmid_launches
    f.restype = ctypes.c_int64
    return int(f())


def mel_for(B, T, seed=0):
    return torch.randn(B, stage_config("s1").mel_channels, T, generator=torch.Generator().manual_seed(seed + 31 * T + B))


def both_paths(monkeypatch, run):
    """run() with the fused launch and with the three launches; checks the path each took."""
    n0 = fused_launches()
    fused = run()
    n1 = fused_launches()
    monkeypatch.setenv("M2_HEADMID", "0")
    three = run()
    n2 = fused_launches()
    monkeypatch.delenv("M2_HEADMID")
    assert n1 > n0 and n2 == n1, (n0, n1, n2)
    return fused, three


@pytest.mark.parametrize("btm", [False, True], ids=["BMT", "BTM"])
@pytest.mark.parametrize("T", [1, 2, 3, 61, 62, 63, 64, 125, 126, 137])
@pytest.mark.parametrize("B", [1, 3])
def test_headmid_bit_equal(gpu, model, monkeypatch, B, T, btm):
    mel = mel_for(B, T).to(gpu)
    if btm:
        mel = mel.transpose(1, 2).contiguous()
    hm = model._hip(gpu)
    fused, three = both_paths(monkeypatch, lambda: hm.vocoder(mel, layout_btm=btm))
    assert fused.shape == (B, 1, 64 * T) and torch.isfinite(fused).all()
    assert torch.equal(fused, three)


def test_headmid_every_rotation(gpu, model, monkeypatch):
    """T = 251: five strips of 201 columns, whose windows start at columns
    -1, 200, 401, 602, 803 = 3, 0, 1, 2, 3 modulo 4 - every rotation of the
    head's planes (the lengths above meet only 1, 2 and 3)."""
    mel = mel_for(2, 251, seed=17).to(gpu)
    fused, three = both_paths(monkeypatch, lambda: model.vocoder(mel))
    assert torch.equal(fused, three)


@pytest.mark.parametrize("T", [2, 63, 137])
def test_headmid_vs_oracle(gpu, model, T):
    mel = mel_for(3, T, seed=7)
    n0 = fused_launches()
    out = model.vocoder(mel.to(gpu)).cpu()
    assert fused_launches() == n0 + 1
    ref = orc.vocoder(golden_state("s1"), mel)
    assert out.shape == ref.shape
    assert rms(out, ref) <= AUDIO_RMS_TOL


@pytest.mark.parametrize("policy", ["fallback", "report"])
def test_headmid_range_policies(gpu, model, monkeypatch, policy):
    """The head's zeroing of the redo's flag and queue words moves into the
    fused kernel: both policies give the three launches' audio."""
    mel = mel_for(3, 64, seed=11).to(gpu)
    model.set_range_policy(policy)
    try:
        fused, three = both_paths(monkeypatch, lambda: model.vocoder(mel))
        again = model.vocoder(mel)
    finally:
        model.set_range_policy("fallback")
    assert torch.isfinite(fused).all()
    assert torch.equal(fused, three) and torch.equal(again, three)


def test_headmid_streamed(gpu, model):
    """Chunks of 16 frames at T = 137, every window on the fused launch:
    bit-identical to the one-shot call."""
    mel = mel_for(2, 137, seed=13).to(gpu)
    full = model.vocoder(mel)
    n0 = fused_launches()
    parts = list(model.vocoder.stream(mel, 16))
    assert fused_launches() == n0 + len(parts) == n0 + 9
    assert torch.equal(torch.cat(parts, dim=2), full)


def test_headmid_not_for_stage2(gpu, monkeypatch):
    from models.tts_model import M2TTSModel
    m = M2TTSModel(**stage_config("s2").as_dict())
    m.load_state_dict(golden_state("s2"))
    m = m.to(gpu).eval()
    mel = torch.randn(2, stage_config("s2").mel_channels, 37, generator=torch.Generator().manual_seed(3))
    n0 = fused_launches()
    out = m.vocoder(mel.to(gpu))
    assert fused_launches() == n0
    monkeypatch.setenv("M2_HEADMID", "0")
    assert torch.equal(m.vocoder(mel.to(gpu)), out)
    assert rms(out.cpu(), orc.vocoder(golden_state("s2"), mel)) <= AUDIO_RMS_TOL


def test_headmid_not_for_device_T(gpu, model, monkeypatch):
    """A speculative back half (the frame count on the device) keeps the three
    launches; the host-T call of the same batch takes the fused one, and the
    two agree bit for bit."""
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 42, (4, 30), generator=g).to(gpu)
    lens = torch.tensor([30, 11, 24, 30]).to(gpu)
    model.inference(ids, lens)  # learns the capacity
    assert model._hip(gpu)._tcap[tuple(ids.shape)] > 0
    n0 = fused_launches()
    mel, audio = model.inference(ids, lens)
    assert fused_launches() == n0
    monkeypatch.setenv("M2_SPECULATIVE", "0")
    hmel, haudio = model.inference(ids, lens)
    assert fused_launches() == n0 + 1
    assert torch.equal(mel, hmel) and torch.equal(audio, haudio)
