#!/usr/bin/env python3
"""Generate tests/golden/dataset_reference.json and dataset_reference.npz from
the reference's own src/data/dataset.py and src/utils/text.py.

Run on the CPU, where the read-only reference tree is (it does not exist on the
GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_dataset_golden.py

The two reference files are loaded under a synthetic package, so that
dataset.py's relative imports resolve; its ``..utils.audio`` is a stand-in
whose ``AudioProcessor.process_file`` reads the WAV, normalises it as
``load_audio(normalize=True)`` does and calls
oracle/audio_oracle.compute_mel_spectrogram (librosa is not installed here;
only the frame count of that mel reaches the recorded fields).

For every variant of dataset_cases.VARIANTS the reference's TTSDataset runs on
the corpus written by dataset_cases.write_corpus, and per sample (sorted by
file name, because the paired layout's order is the file system's) the text,
ids, ``text_length``, ``mel_length`` and durations are recorded, with
``collate_fn`` of the items in that order (the mel values are left out: only
their shape).  ``torch.manual_seed(DUMMY_SEED); DummyDataset(*DUMMY_ARGS)``
items and their collated batch go into the .npz.  Only data is written.
"""
import importlib.util
import json
import os
import sys
import tempfile
import types
import wave
from pathlib import Path

import numpy as np
import torch

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
REF_SRC = Path(os.environ.get("M2TTS_REFERENCE", "/root/reference")) / "src"
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent / "oracle"))

import audio_oracle as ao  # noqa: E402
import dataset_cases as dc  # noqa: E402

PKG = "reference_src"


class StandInAudioProcessor:
    """What dataset.py needs of ..utils.audio.AudioProcessor, on the oracle."""

    def __init__(self, sample_rate=22050, n_fft=1024, hop_length=256, win_length=1024, n_mels=64, fmin=0, fmax=None):
        self.args = (sample_rate, n_fft, hop_length, win_length, n_mels, fmin, fmax or sample_rate // 2)

    def process_file(self, audio_path):
        with wave.open(str(audio_path), "rb") as w:
            assert w.getframerate() == self.args[0]
            y = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.float32) / np.float32(32768.0)
        m = np.max(np.abs(y))
        y = y / m if m > 0 else y
        return y, ao.compute_mel_spectrogram(y, *self.args)


def load_reference():
    """reference_src.data.dataset with reference_src.utils.text from the
    reference tree and the stand-in reference_src.utils.audio."""
    for name in (PKG, PKG + ".utils", PKG + ".data"):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    audio = types.ModuleType(PKG + ".utils.audio")
    audio.AudioProcessor = StandInAudioProcessor
    sys.modules[audio.__name__] = audio
    for name, path in ((PKG + ".utils.text", REF_SRC / "utils" / "text.py"),
                       (PKG + ".data.dataset", REF_SRC / "data" / "dataset.py")):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[PKG + ".data.dataset"]


def collated(batch):
    return {"phoneme_ids": batch["phoneme_ids"].tolist(), "text_lengths": batch["text_lengths"].tolist(),
            "mel_lengths": batch["mel_lengths"].tolist(), "durations": batch["durations"].double().tolist(),
            "mel_specs_shape": list(batch["mel_specs"].shape), "texts": batch["texts"]}


def main():
    ref = load_reference()
    out = {"variants": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (layout, kwargs) in dc.VARIANTS.items():
            root = dc.write_corpus(Path(tmp) / name, layout)
            ds = ref.TTSDataset(root, max_text_length=dc.MAX_TEXT_LENGTH, **kwargs)
            order = sorted(range(len(ds)), key=lambda i: Path(ds.samples[i]["audio_path"]).name)
            samples = []
            for i in order:
                s = ds.samples[i]
                assert s["mel_spec"].dtype == np.float32 and s["mel_spec"].shape == (dc.N_MELS, s["mel_length"])
                samples.append({"name": Path(s["audio_path"]).stem, "text": s["text"],
                                "phoneme_ids": [int(v) for v in s["phoneme_ids"]], "phonemes": list(s["phonemes"]),
                                "text_length": int(s["text_length"]), "mel_length": int(s["mel_length"]),
                                "durations": [float(v) for v in s["durations"]]})
            out["variants"][name] = {"samples": samples, "collate": collated(ref.collate_fn([ds[i] for i in order]))}
    arrays = {}
    torch.manual_seed(dc.DUMMY_SEED)
    dummy = ref.DummyDataset(*dc.DUMMY_ARGS)
    items = [dummy[i] for i in range(len(dummy))]
    for i, it in enumerate(items):
        for k in ("phoneme_ids", "text_length", "mel_spec", "mel_length", "durations"):
            arrays[f"item{i}_{k}"] = it[k].numpy()
    out["dummy_texts"] = [it["text"] for it in items]
    batch = ref.collate_fn(items)
    for k in ("phoneme_ids", "text_lengths", "mel_specs", "mel_lengths", "durations"):
        arrays[f"batch_{k}"] = batch[k].numpy()
    out["exports"] = sorted(n for n in ("TTSDataset", "collate_fn", "create_dataloader", "DummyDataset")
                            if hasattr(ref, n))
    (HERE / "dataset_reference.json").write_text(json.dumps(out, indent=1) + "\n")
    np.savez_compressed(HERE / "dataset_reference.npz", **arrays)
    print({k: [(s["name"], s["mel_length"]) for s in v["samples"]] for k, v in out["variants"].items()})


if __name__ == "__main__":
    main()
