"""Ragged batches: every utterance of M2TTSModel.inference_ragged equals the
single-utterance call on it, and everything past its end is zero.

Expected values: the CPU oracle run per utterance (oracle/m2tts_oracle.py,
bit-identical to the reference on CPU), under the project's parity bar (mel
max-abs <= 1e-3, waveform RMS <= 1e-4, waveform max-abs <= 1e-3) applied to
each utterance's valid region alone.  Frame counts and the padding are exact.
"""
import functools
import sys
import wave

import numpy as np
import pytest
import torch

import m2tts_oracle as orc
from conftest import AUDIO_RMS_TOL, MEL_MAXABS_TOL, ROOT, golden_state, maxabs, rms, stage_config

pytestmark = pytest.mark.gpu
STAGES = ["s1", "s2"]
AUDIO_MAXABS_TOL = 1e-3  # as test_gpu_parity.test_inference_small

# B=4, S=12: integer durations with totals 97 (a bound inside a 64-row tile),
# 64 (exactly a tile edge), 33 (one past a 32-key chunk) and 0 (the reference's
# single zero row, T_b = 1); utterance 1 has a shortened length.
FRAMES = (97, 64, 33, 1)
B, S = 4, 12


def _case():
    g = torch.Generator().manual_seed(20)
    ids = torch.randint(1, 40, (B, S), generator=g)
    lens = torch.tensor([12, 7, 12, 12])
    d = torch.zeros(B, S)
    d[0] = torch.tensor([9.] + [8.] * 11)
    d[1] = torch.tensor([6.] * 4 + [5.] * 8)
    d[2] = torch.tensor([3.] * 9 + [2.] * 3)
    assert tuple(int(x) for x in d.sum(1)) == (97, 64, 33, 0)
    return ids, lens, d


@functools.lru_cache(maxsize=None)
def _model(stage):
    from models.tts_model import M2TTSModel
    m = M2TTSModel(**stage_config(stage).as_dict())
    m.load_state_dict(golden_state(stage))
    return m.to(torch.device("cuda:0")).eval()


@functools.lru_cache(maxsize=None)
def _reference(stage):
    """The oracle's single-utterance (mel [T_b, M], audio [64 T_b]) of the case, computed once."""
    ids, lens, d = _case()
    sd, cfg = golden_state(stage), stage_config(stage)
    out = []
    for b in range(B):
        r = orc.forward(sd, cfg, ids[b:b + 1], lens[b:b + 1], target_durations=d[b:b + 1])
        assert r["mel_output"].shape[1] == FRAMES[b]
        out.append((r["mel_output"][0], r["audio_output"][0, 0]))
    return out


def _check_valid(mel, audio, frames, want, stage=""):
    mel, audio = mel.cpu(), audio.cpu()
    for b, (rm, ra) in enumerate(want):
        t = int(frames[b])
        assert t == rm.shape[0]
        e_mel, e_rms, e_max = maxabs(mel[b, :t], rm), rms(audio[b, 0, :64 * t], ra), maxabs(audio[b, 0, :64 * t], ra)
        print(f"{stage} utterance {b} T_b={t}: mel max-abs {e_mel:.3e}, audio rms {e_rms:.3e} max-abs {e_max:.3e}")
        assert e_mel <= MEL_MAXABS_TOL, (b, e_mel)
        assert e_rms <= AUDIO_RMS_TOL, (b, e_rms)
        assert e_max <= AUDIO_MAXABS_TOL, (b, e_max)


def _check_padding(mel, audio, frames):
    for b in range(mel.shape[0]):
        t = int(frames[b])
        assert torch.count_nonzero(mel[b, t:]) == 0, b
        assert torch.count_nonzero(audio[b, 0, 64 * t:]) == 0, b
    assert bool(torch.isfinite(mel).all()) and bool(torch.isfinite(audio).all())


def _run_case(stage, gpu):
    ids, lens, d = _case()
    m = _model(stage)
    mel, audio, frames = m.inference_ragged(ids.to(gpu), lens.to(gpu), durations=d.to(gpu))
    assert frames.dtype == torch.int64 and frames.device.type == "cuda"
    assert tuple(frames.tolist()) == FRAMES
    tmax, M = max(FRAMES), stage_config(stage).mel_channels
    assert mel.shape == (B, tmax, M) and audio.shape == (B, 1, 64 * tmax)
    _check_valid(mel, audio, frames, _reference(stage), stage)
    _check_padding(mel, audio, frames)
    return mel, audio, frames


@pytest.mark.parametrize("stage", STAGES)
def test_end_to_end(gpu, stage):
    from models.tts_model import unpad
    mel, audio, frames = _run_case(stage, gpu)
    parts = unpad(mel, audio, frames)
    assert [tuple(p[0].shape) for p in parts] == [(t, mel.shape[2]) for t in FRAMES]
    assert [tuple(p[1].shape) for p in parts] == [(64 * t,) for t in FRAMES]
    assert parts[0][0].data_ptr() == mel.data_ptr()  # views


QS2 = [None, "0", "2", "3", "4", "12"]


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("qs2", QS2)
@pytest.mark.parametrize("rb", ["1", "2", "4"])
def test_every_tile_form(gpu, stage, rb, qs2, monkeypatch):
    """16-, 32- and 64-row tiles, each 64-row attention form."""
    monkeypatch.setenv("M2_TFL_RB", rb)
    if qs2 is None:
        monkeypatch.delenv("M2_TFL_QS2", raising=False)
    else:
        monkeypatch.setenv("M2_TFL_QS2", qs2)
    mel, _, frames = _run_case(stage, gpu)
    if rb == "1":
        # the same 16-row form and operation sequence as the B=1 call: the
        # utterance's rows and keys are bounded by T_b in both
        ids, lens, d = _case()
        m = _model(stage)
        for b in range(B):
            one = m(ids[b:b + 1].to(gpu), lens[b:b + 1].to(gpu), target_durations=d[b:b + 1].to(gpu))["mel_output"]
            assert torch.equal(mel[b, :FRAMES[b]], one[0]), b


@pytest.mark.parametrize("stage", STAGES)
def test_first_launch_64_row_tiles(gpu, stage, monkeypatch):
    monkeypatch.setenv("M2_TFL_FIRST_RB", "4")
    _run_case(stage, gpu)


@pytest.mark.parametrize("stage", STAGES)
def test_fallback_without_one_launch_layers(gpu, stage, monkeypatch):
    """M2_TF_LAYER=0: the entry points answer M2_E_SHAPE and inference_ragged
    runs the utterances one by one."""
    from m2amd import _lib
    monkeypatch.setenv("M2_TF_LAYER", "0")
    ids, lens, d = _case()
    hm = _model(stage)._hip(gpu)
    with pytest.raises(_lib.M2Error) as e:
        hm.inference_ragged(ids.to(gpu), lens.to(gpu), 1.0, d.to(gpu))
    assert e.value.status == _lib.M2_E_SHAPE
    _run_case(stage, gpu)


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("scale", [1.0, 1.3])
def test_uniform_lengths_equal_inference(gpu, stage, scale):
    """Pinned durations: every utterance has the same T_b (5 S at scale 1), so
    the ragged call is the plain one, bit for bit."""
    g = torch.Generator().manual_seed(21)
    ids = torch.randint(1, 40, (2, 24), generator=g).to(gpu)
    lens = torch.tensor([24, 17]).to(gpu)
    m = _model(stage)
    mel, audio, frames = m.inference_ragged(ids, lens, duration_scale=scale)
    want_mel, want_audio = m.inference(ids, lens, duration_scale=scale)
    assert frames.tolist() == [want_mel.shape[1]] * 2
    if scale == 1.0:
        assert want_mel.shape[1] == 5 * 24
    assert torch.equal(mel, want_mel) and torch.equal(audio, want_audio)


def _fresh_model(stage, gpu):
    from models.tts_model import M2TTSModel
    m = M2TTSModel(**stage_config(stage).as_dict())
    m.load_state_dict(golden_state(stage))
    return m.to(gpu).eval()


VOC_FRAMES = (40, 39, 37, 5, 2, 1)


@functools.lru_cache(maxsize=None)
def _vocoder_case(stage):
    M = stage_config(stage).mel_channels
    mel = torch.rand(6, 40, M, generator=torch.Generator().manual_seed(22)) * 2 - 1
    sd = golden_state(stage)
    want = [orc.vocoder(sd, mel[b:b + 1, :t].transpose(1, 2))[0, 0] for b, t in enumerate(VOC_FRAMES)]
    return mel, want


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("precision", ["split", "f32"])
def test_vocoder_alone(gpu, stage, precision):
    """m2_vocoder_ragged: the end window of T_b = 40 is skipped, 39 and 37
    recompute 3 frames next to the batch's end, 5 / 2 / 1 are utterances
    shorter than the window; then streamed in 16-frame chunks, and once in the
    [B, M, T] layout."""
    mel, want = _vocoder_case(stage)
    m = _fresh_model(stage, gpu)
    m.set_vocoder_precision(precision)
    hm = m._hip(gpu)
    assert hm.vocoder_path() == {"split": 2, "f32": 1}[precision]
    frames = torch.tensor(VOC_FRAMES, dtype=torch.int32, device=gpu)

    def check(audio, what):
        assert audio.shape == (6, 1, 64 * 40)
        audio = audio.cpu()
        for b, t in enumerate(VOC_FRAMES):
            e_rms, e_max = rms(audio[b, 0, :64 * t], want[b]), maxabs(audio[b, 0, :64 * t], want[b])
            print(f"{stage} {precision} {what} T_b={t}: audio rms {e_rms:.3e} max-abs {e_max:.3e}")
            assert e_rms <= AUDIO_RMS_TOL and e_max <= AUDIO_MAXABS_TOL, (what, b, e_rms, e_max)
            assert torch.count_nonzero(audio[b, 0, 64 * t:]) == 0, (what, b)

    check(hm.vocoder_ragged(mel.to(gpu), frames, layout_btm=True), "whole")
    check(hm.vocoder_ragged(mel.transpose(1, 2).contiguous().to(gpu), frames, layout_btm=False), "[B,M,T]")
    m.set_vocoder_chunking(16)
    check(hm.vocoder_ragged(mel.to(gpu), frames, layout_btm=True), "chunked")


@pytest.mark.parametrize("stage", STAGES)
def test_decoder_alone(gpu, stage):
    """m2_mel_decoder_ragged on rows that are not a frame expansion."""
    cfg, sd = stage_config(stage), golden_state(stage)
    x = torch.randn(3, 70, cfg.hidden_dim, generator=torch.Generator().manual_seed(23))
    counts = (70, 17, 1)
    hm = _model(stage)._hip(gpu)
    mel = hm.decoder_ragged(x.to(gpu), torch.tensor(counts, dtype=torch.int32, device=gpu)).cpu()
    assert mel.shape == (3, 70, cfg.mel_channels)
    for b, t in enumerate(counts):
        err = maxabs(mel[b, :t], orc.mel_decoder(sd, cfg, x[b:b + 1, :t])[0])
        print(f"{stage} decoder T_b={t}: mel max-abs {err:.3e}")
        assert err <= MEL_MAXABS_TOL, (b, err)
        assert torch.count_nonzero(mel[b, t:]) == 0, b


def _pcm(path):
    with wave.open(str(path)) as w:
        assert (w.getnchannels(), w.getsampwidth()) == (1, 2)
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.int32)


@pytest.mark.parametrize("pinned", [True, False])
def test_cli_text_file(gpu, tmp_path, pinned):
    """--text-file writes one WAV per line, each the WAV the single-text path
    writes for that line (within 1 LSB).  Pinned durations: 1280 frames per
    text; the untrained projection: the one zero frame."""
    sys.path.insert(0, str(ROOT / "m2-tts_amd" / "scripts"))
    import synthesize
    ck = tmp_path / "stage1.pt"
    cfg = {"model": {"text_encoder": {"vocab_size": 256, "hidden_dim": 64, "num_layers": 2, "num_heads": 2,
                                      "dropout": 0.1}, "decoder": {"mel_channels": 64, "num_layers": 2},
                     "vocoder": {"hidden_channels": 128}}}
    torch.save({"model_state_dict": golden_state("s1", pinned), "config": cfg, "step": 1}, ck)
    texts = ["Hello world.", "The quick brown fox jumps over the lazy dog.", "Testing one two three"]
    tf = tmp_path / "texts.txt"
    tf.write_text(texts[0] + "\n\n" + texts[1] + "\n   \n" + texts[2] + "\n")
    out = tmp_path / "batch"
    synthesize.main(["--text-file", str(tf), "--checkpoint", str(ck), "--output-dir", str(out)])
    assert sorted(p.name for p in out.iterdir()) == ["00000.wav", "00001.wav", "00002.wav"]
    for i, text in enumerate(texts):
        single = tmp_path / f"single{i}.wav"
        synthesize.main(["--text", text, "--checkpoint", str(ck), "--output", str(single)])
        got, want = _pcm(out / f"{i:05d}.wav"), _pcm(single)
        assert got.shape == want.shape == (64 * (1280 if pinned else 1),)
        assert int(np.abs(got - want).max()) <= 1, i
