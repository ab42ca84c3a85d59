"""GPU: ResBlock1's item map in the stage1 16-wave planar head (M2_HEAD_ITEMS,
default 1: the four waves of an m-block are consecutive waves, one on every
SIMD; 0: the ConvT1 map, the four waves of one SIMD) and the weight hand-over
from the head's last layer into the mid roles of headmid_kernel.  Every item
computes the same sums in the same order under both maps, and the hand-over
only starts loads earlier, so the audio is equal bit for bit: between the two
maps on the fused launch and on the three launches (x3_head_kernel runs the
same function), and between the default build and M2_HEADMID=0.  Lengths as in
test_gpu_headmid.py: one window holding both utterance edges (T = 1, 2, 3), a
strip at and across the 252 valid positions of a window (61 .. 64), two full
strips (125), a ragged last strip (126, 137).
"""
import ctypes

import pytest
import torch

import m2tts_oracle as orc
from conftest import AUDIO_RMS_TOL, golden_state, rms, stage_config

pytestmark = pytest.mark.gpu

S_MAX = 250  # headmid_kernel: owned columns of U1 per strip (kHeadmidSMax, vocoder_launch.h)


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


def both_maps(monkeypatch, run):
    """run() under M2_HEAD_ITEMS=1 and =0."""
    monkeypatch.setenv("M2_HEAD_ITEMS", "1")
    new = run()
    monkeypatch.setenv("M2_HEAD_ITEMS", "0")
    old = run()
    monkeypatch.delenv("M2_HEAD_ITEMS")
    return new, old


@pytest.mark.parametrize("headmid", ["0", "1"], ids=["three", "fused"])
@pytest.mark.parametrize("btm", [False, True], ids=["BMT", "BTM"])
@pytest.mark.parametrize("T", [1, 2, 3, 61, 62, 63, 64, 125, 126, 137])
@pytest.mark.parametrize("B", [1, 3])
def test_head_items_bit_equal(gpu, model, monkeypatch, B, T, btm, headmid):
    mel = mel_for(B, T).to(gpu)
    if btm:
        mel = mel.transpose(1, 2).contiguous()
    hm = model._hip(gpu)
    monkeypatch.setenv("M2_HEADMID", headmid)
    n0 = fused_launches()
    new, old = both_maps(monkeypatch, lambda: hm.vocoder(mel, layout_btm=btm))
    assert fused_launches() - n0 == (2 if headmid == "1" else 0)  # the path each call took
    assert new.shape == (B, 1, 64 * T) and torch.isfinite(new).all()
    assert torch.equal(new, old)


ROT_T = 251  # five strips of 201 columns: windows start at columns -1, 200, 401, 602, 803


@pytest.fixture(scope="module")
def rotations(gpu, model):
    """The T = 251 batch of test_headmid_every_rotation, once: the default
    build (fused launch, default item map) and the three launches."""
    from m2amd import _lib
    mel = mel_for(2, ROT_T, seed=17).to(gpu)
    mp = pytest.MonkeyPatch()
    try:
        n0 = fused_launches()
        fused = model.vocoder(mel)
        assert fused_launches() == n0 + 1
        mp.setenv("M2_HEADMID", "0")
        _lib.reload_switches()
        three = model.vocoder(mel)
        assert fused_launches() == n0 + 1
    finally:
        mp.undo()
        _lib.reload_switches()
    return fused, three


@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_every_rotation_equals_three_launches(rotations, rot):
    """The strips whose window starts at `rot` modulo 4 (the rotation of the
    head's planes): their 16 audio samples per owned U1 column.  No strip has
    16 chunks (S = 201: 13), and the last one is ragged (200 columns)."""
    fused, three = rotations
    L1 = 4 * ROT_T
    n = -(-L1 // S_MAX)
    S = -(-L1 // n)
    assert (n, S) == (5, 201)
    strips = [k for k in range(n) if (k * S - 1) % 4 == rot]
    assert strips, rot
    for k in strips:
        a, b = 16 * k * S, 16 * min(L1, (k + 1) * S)
        assert torch.equal(fused[:, :, a:b], three[:, :, a:b]), (rot, k)


@pytest.mark.parametrize("T", [1, 5, 16])
def test_shorter_than_one_strip_equals_three_launches(gpu, model, monkeypatch, T):
    """One strip of 4 T < 250 columns (nch = 1, 2, 4): the roles' handed-over
    weights against the three launches' own fetches."""
    mel = mel_for(2, T, seed=23).to(gpu)
    n0 = fused_launches()
    fused = model.vocoder(mel)
    assert fused_launches() == n0 + 1
    monkeypatch.setenv("M2_HEADMID", "0")
    three = model.vocoder(mel)
    assert fused_launches() == n0 + 1
    assert torch.equal(fused, three)


@pytest.mark.parametrize("T", [2, 63, 137])
def test_head_items_vs_oracle(gpu, model, T):
    mel = mel_for(3, T, seed=7)
    n0 = fused_launches()
    out = model.vocoder(mel.to(gpu)).cpu()
    assert fused_launches() == n0 + 1
    ref = orc.vocoder(golden_state("s1"), mel)
    assert out.shape == ref.shape
    assert rms(out, ref) <= AUDIO_RMS_TOL
