"""GPU: AudioProcessor.process_files and data.dataset.TTSDataset on the
three-file corpus of tests/golden/dataset_cases.py, written into tmp_path.

process_files must give what process_file gives per file, bit for bit, however
the files are split into calls.  TTSDataset's non-mel fields must equal what
the reference's own dataset.py recorded (tests/golden/make_dataset_golden.py),
and its mel must be within audio_cases.mel_bound of the float64 oracle of the
whole file, truncation included."""
import json
import pickle
import sys

import numpy as np
import pytest
import torch

import audio_cases as ac

from conftest import GOLDEN

if str(GOLDEN) not in sys.path:
    sys.path.insert(0, str(GOLDEN))

import dataset_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu

HANDLES = [(22050, 1024, 256, 1024, 64, 0, 11025), ac.CONFIGS[1], ac.CONFIGS[5]]


@pytest.fixture(scope="module")
def ref():
    return json.loads((GOLDEN / "dataset_reference.json").read_text())


def _same(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("cfg", HANDLES, ids=ac.config_id)
def test_process_files_equals_process_file(gpu, cfg, tmp_path):
    from utils.audio import AudioProcessor
    root = dc.write_corpus(tmp_path / "corpus", "paired")
    paths = [root / f"{n}.wav" for n in dc.NAMES]
    ap = AudioProcessor(*cfg)
    single = [ap.process_file(p) for p in paths]
    for (audio, mel), n in zip(single, dc.NAMES):
        assert mel.shape == (cfg[4], 1 + len(audio) // cfg[2]) and _same(audio, dc.normalised(n))
    batch = ap.process_files(paths)
    assert len(batch) == 3
    for (a1, m1), (a2, m2) in zip(single, batch):
        assert _same(a1, a2) and _same(m1, m2) and m2.flags["C_CONTIGUOUS"]
    one = ap.process_files([paths[1]])
    assert len(one) == 1 and _same(one[0][0], single[1][0]) and _same(one[0][1], single[1][1])
    # a budget below every file: each file is its own call
    smallest = min(len(a) for a, _ in single)
    apart = ap.process_files(paths, sample_budget=smallest - 1)
    # a budget that holds the first two files but not the third
    two = ap.process_files(paths, sample_budget=len(single[0][0]) + len(single[1][0]))
    for (a1, m1), (a2, m2), (a3, m3) in zip(batch, apart, two):
        assert _same(a1, a2) and _same(m1, m2) and _same(a1, a3) and _same(m1, m3)
    cut = ap.process_files(paths, max_mel_length=7, return_audio=False)
    for (_, m1), (a2, m2) in zip(batch, cut):
        assert a2 is None and _same(np.ascontiguousarray(m1[:, :7]), m2)


def test_process_files_drops_only_the_failing_file(gpu, tmp_path):
    from utils.audio import AudioProcessor
    root = dc.write_corpus(tmp_path / "corpus", "paired")
    (root / "broken.wav").write_bytes(b"not a RIFF file")
    dc.write_pcm16(root / "empty.wav", np.zeros(0, "<i2"))
    dc.write_pcm16(root / "other_rate.wav", dc.to_pcm16(dc.signal("utt_c")), 16000)
    names = ["utt_a", "broken", "utt_b", "empty", "missing", "other_rate", "utt_c"]
    ap = AudioProcessor()
    got = ap.process_files([root / f"{n}.wav" for n in names])
    assert [g is None for g in got] == [False, True, False, True, True, True, False]
    for n, g in zip(names, got):
        if g is not None:
            audio, mel = ap.process_file(root / f"{n}.wav")
            assert _same(g[0], audio) and _same(g[1], mel)
    with pytest.raises(ValueError):
        ap.process_file(root / "other_rate.wav")  # process_file itself still raises
    assert ap.process_files([]) == [] and ap.process_files([root / "missing.wav"]) == [None]


def _by_name(samples):
    from pathlib import Path
    return sorted(samples, key=lambda s: Path(s["audio_path"]).name)


@pytest.mark.parametrize("variant", list(dc.VARIANTS))
def test_tts_dataset_equals_the_reference(gpu, ref, variant, tmp_path):
    from data.dataset import TTSDataset, collate_fn
    from pathlib import Path
    layout, kwargs = dc.VARIANTS[variant]
    root = dc.write_corpus(tmp_path / variant, layout)
    if layout == "paired":  # found and skipped: no decoder; and an unreadable file drops only itself
        (root / "song.mp3").write_bytes(b"ID3")
        (root / "song.txt").write_text("a song\n")
        (root / "zz_broken.wav").write_bytes(b"RIFF")
        (root / "zz_broken.txt").write_text("broken\n")
    cache = tmp_path / "cache"
    data = TTSDataset(root, max_text_length=dc.MAX_TEXT_LENGTH, cache_dir=cache, **kwargs)
    want = ref["variants"][variant]
    assert len(data) == len(want["samples"])
    if layout == "ljspeech":  # metadata order; the paired layout's order is the file system's
        assert [Path(s["audio_path"]).stem for s in data.samples] == [s["name"] for s in want["samples"]]
    samples = _by_name(data.samples)
    worst = 0.0
    for s, w in zip(samples, want["samples"]):
        assert set(s) == {"audio_path", "text", "phoneme_ids", "phonemes", "text_length", "mel_spec", "mel_length",
                          "durations"}
        assert Path(s["audio_path"]).stem == w["name"] and isinstance(s["audio_path"], str)
        for k in ("text", "phoneme_ids", "phonemes", "text_length", "mel_length", "durations"):
            assert s[k] == w[k] and type(s[k]) is type(w[k]), (w["name"], k)
        mel = s["mel_spec"]
        assert isinstance(mel, np.ndarray) and mel.dtype == np.float32 and mel.shape == (dc.N_MELS, w["mel_length"])
        y = dc.normalised(w["name"])
        bound, _ = ac.mel_bound(y, dc.CFG)
        assert bound == 1e-3
        oracle = ac.mel_reference(y, dc.CFG)[2][:, :w["mel_length"]]  # the whole file's features, then cut
        err = float(np.abs(mel - oracle).max())
        worst = max(worst, err)
        assert err <= bound, (w["name"], err)
    print(f"DATASET mel_vs_float64 {variant} {worst:.3e}")
    order = sorted(range(len(data)), key=lambda i: Path(data.samples[i]["audio_path"]).name)
    items = [data[i] for i in order]
    for it, w in zip(items, want["samples"]):
        assert it["mel_spec"].dtype == torch.float32 and it["mel_spec"].is_contiguous()
        assert it["mel_spec"].device.type == "cpu" and it["mel_spec"].shape == (dc.N_MELS, w["mel_length"])
        assert it["phoneme_ids"].dtype == it["text_length"].dtype == it["mel_length"].dtype == torch.int64
        assert it["durations"].dtype == torch.float32 and it["durations"].shape == (w["text_length"],)
    batch, wc = collate_fn(items), want["collate"]
    assert batch["phoneme_ids"].tolist() == wc["phoneme_ids"] and batch["text_lengths"].tolist() == wc["text_lengths"]
    assert batch["mel_lengths"].tolist() == wc["mel_lengths"] and batch["texts"] == wc["texts"]
    assert batch["durations"].double().tolist() == wc["durations"]
    assert list(batch["mel_specs"].shape) == wc["mel_specs_shape"]
    # the cache, written and re-read (the corpus is not needed any more)
    with open(cache / "processed_samples.pkl", "rb") as f:
        stored = pickle.load(f)
    assert isinstance(stored, list) and len(stored) == len(data)
    again = TTSDataset(tmp_path / "gone", max_text_length=dc.MAX_TEXT_LENGTH, cache_dir=cache, **kwargs)
    assert len(again) == len(data)
    for s, t in zip(data.samples, again.samples):
        assert {k: v for k, v in s.items() if k != "mel_spec"} == {k: v for k, v in t.items() if k != "mel_spec"}
        assert _same(np.ascontiguousarray(s["mel_spec"]), np.ascontiguousarray(t["mel_spec"]))
