"""data.dataset on the host: DummyDataset, collate_fn, the uniform alignment,
the cache structure and the loader against what the reference's own
src/data/dataset.py gave (tests/golden/make_dataset_golden.py).  No GPU and no
loader workers."""
import inspect
import json
import pickle
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

if str(GOLDEN) not in sys.path:
    sys.path.insert(0, str(GOLDEN))

import dataset_cases as dc  # noqa: E402

from data import dataset as ds  # noqa: E402

ITEM_KEYS = ("phoneme_ids", "text_length", "mel_spec", "mel_length", "durations")
BATCH_KEYS = ("phoneme_ids", "text_lengths", "mel_specs", "mel_lengths", "durations")


@pytest.fixture(scope="module")
def ref():
    return json.loads((GOLDEN / "dataset_reference.json").read_text())


@pytest.fixture(scope="module")
def arrays():
    return np.load(GOLDEN / "dataset_reference.npz", allow_pickle=False)


def dummy_items():
    torch.manual_seed(dc.DUMMY_SEED)
    d = ds.DummyDataset(*dc.DUMMY_ARGS)
    return [d[i] for i in range(len(d))]


def same(t, a):
    t = t.numpy()
    return t.dtype == a.dtype and t.shape == a.shape and np.array_equal(t, a)


def test_module_exports_the_reference_names(ref):
    assert ref["exports"] == sorted(("TTSDataset", "collate_fn", "create_dataloader", "DummyDataset"))
    for name in ref["exports"]:
        assert hasattr(ds, name), name
    sig = inspect.signature(ds.TTSDataset.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[2:]] == [
        ("subset_size", None), ("max_text_length", 256), ("max_mel_length", 1000), ("sample_rate", 22050),
        ("n_mels", 64), ("cache_dir", None)]
    sig = inspect.signature(ds.create_dataloader)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("batch_size", 2), ("shuffle", True), ("num_workers", 2), ("pin_memory", False), ("drop_last", True)]
    sig = inspect.signature(ds.DummyDataset.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("size", 100), ("max_text_length", 50), ("max_mel_length", 200), ("mel_dim", 64), ("vocab_size", 256)]


def test_dummy_dataset_equals_the_reference(ref, arrays):
    items = dummy_items()
    assert len(items) == dc.DUMMY_ARGS[0]
    assert [it["text"] for it in items] == ref["dummy_texts"]
    for i, it in enumerate(items):
        assert set(it) == set(ITEM_KEYS) | {"text"}
        for k in ITEM_KEYS:
            assert same(it[k], arrays[f"item{i}_{k}"]), (i, k)


def test_collate_fn_equals_the_reference(arrays):
    batch = ds.collate_fn(dummy_items())
    assert set(batch) == set(BATCH_KEYS) | {"texts"}
    for k in BATCH_KEYS:
        assert same(batch[k], arrays[f"batch_{k}"]), k
    # the layout the ragged feature kernel writes: zeros behind every utterance's frames
    for b, n in enumerate(batch["mel_lengths"].tolist()):
        assert not batch["mel_specs"][b, :, n:].any()


def test_uniform_durations_equal_the_reference(ref):
    from utils.text import TextProcessor
    tp = TextProcessor()
    seen = set()
    for name, v in ref["variants"].items():
        for s in v["samples"]:
            info = tp.process_text(s["text"], dc.MAX_TEXT_LENGTH)
            assert info["phoneme_ids"] == s["phoneme_ids"] and info["phonemes"] == s["phonemes"]
            assert len(info["phoneme_ids"]) == s["text_length"] == dc.MAX_TEXT_LENGTH  # the padded length
            assert info["length"] == sum(p != "SIL" for p in s["phonemes"]) < s["text_length"]
            got = ds.uniform_durations(s["mel_length"], info["length"], len(info["phoneme_ids"]))
            assert got == s["durations"], (name, s["name"])  # Python floats, exactly
            seen.add((s["mel_length"], info["length"]))
    assert len(seen) >= 5
    # reference dataset.py:186-196: no non-SIL phoneme -> all zeros; more phonemes than ids -> cut
    assert ds.uniform_durations(36, 0, 4) == [0.0] * 4
    assert ds.uniform_durations(9, 6, 4) == [1.5] * 4
    assert ds.uniform_durations(7, 3, 3) == [7 / 3] * 3


def test_create_dataloader_without_workers_yields_batches():
    torch.manual_seed(3)
    loader = ds.create_dataloader(ds.DummyDataset(5, 12, 60, 8, 50), batch_size=2, shuffle=False, num_workers=0)
    batches = list(loader)
    assert len(batches) == 2  # drop_last
    for b in batches:
        assert b["phoneme_ids"].shape[0] == 2 and b["mel_specs"].shape[:2] == (2, 8)
        assert b["mel_specs"].shape[2] == int(b["mel_lengths"].max())
        assert len(b["texts"]) == 2
    assert loader.collate_fn is ds.collate_fn and loader.num_workers == 0


def test_create_dataloader_with_workers_is_configured_as_the_reference(monkeypatch):
    """The arguments only: no worker is started."""
    seen = {}

    def fake(dataset, **kw):
        seen.update(kw)
        return "loader"

    monkeypatch.setattr(ds, "DataLoader", fake)
    assert ds.create_dataloader(ds.DummyDataset(4), num_workers=2) == "loader"
    assert seen["persistent_workers"] is True and seen["prefetch_factor"] == 1
    assert (seen["batch_size"], seen["shuffle"], seen["num_workers"], seen["pin_memory"], seen["drop_last"]) == (
        2, True, 2, False, True)
    seen.clear()
    ds.create_dataloader(ds.DummyDataset(4), num_workers=0)
    assert "prefetch_factor" not in seen and not seen.get("persistent_workers", False)


def test_reference_made_cache_loads(ref, tmp_path):
    """processed_samples.pkl as the reference writes it: a list of dictionaries
    of plain Python values and a float32 mel (here zeros of the recorded shape)."""
    samples = []
    for s in ref["variants"]["lj"]["samples"]:
        samples.append({"audio_path": f"/corpus/wavs/{s['name']}.wav", "text": s["text"],
                        "phoneme_ids": s["phoneme_ids"], "phonemes": s["phonemes"], "text_length": s["text_length"],
                        "mel_spec": np.zeros((dc.N_MELS, s["mel_length"]), np.float32), "mel_length": s["mel_length"],
                        "durations": s["durations"]})
    cache = tmp_path / "cache"
    cache.mkdir()
    with open(cache / "processed_samples.pkl", "wb") as f:
        pickle.dump(samples, f)
    data = ds.TTSDataset(tmp_path / "no_such_corpus", subset_size=2, cache_dir=cache)  # never reaches the GPU
    assert len(data) == 2
    want = ref["variants"]["lj_subset"]["collate"]
    items = [data[i] for i in range(len(data))]
    for it, s in zip(items, samples):
        assert it["phoneme_ids"].dtype == torch.int64 and it["phoneme_ids"].tolist() == s["phoneme_ids"]
        assert it["text_length"].dtype == torch.int64 and it["text_length"].tolist() == [s["text_length"]]
        assert it["mel_length"].dtype == torch.int64 and it["mel_length"].tolist() == [s["mel_length"]]
        assert it["mel_spec"].dtype == torch.float32 and it["mel_spec"].shape == (dc.N_MELS, s["mel_length"])
        assert it["durations"].dtype == torch.float32
        assert it["durations"].tolist() == torch.tensor(s["durations"], dtype=torch.float32).tolist()
        assert it["text"] == s["text"]
    batch = ds.collate_fn(items)
    assert batch["phoneme_ids"].tolist() == want["phoneme_ids"]
    assert batch["text_lengths"].tolist() == want["text_lengths"]
    assert batch["mel_lengths"].tolist() == want["mel_lengths"]
    assert batch["durations"].double().tolist() == want["durations"]
    assert list(batch["mel_specs"].shape) == want["mel_specs_shape"] and batch["texts"] == want["texts"]
