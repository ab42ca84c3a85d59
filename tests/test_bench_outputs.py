"""bench.py's plain form: ``--full`` is opt-in, ``--steps`` is the number of
timed steps, and ``--dump-outputs`` writes what the last timed step returned
(float32 .npy, a fixed seeded sample when an array is over its share)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def test_full_and_dump_are_opt_in():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    g = torch.Generator().manual_seed(3)
    mel, audio = torch.randn(4, 50, 8, generator=g), torch.randn(4, 1, 3200, generator=g).double()
    bench.dump_outputs(str(tmp_path / "whole"), [("mel", mel), ("audio", audio)])
    m, a = np.load(tmp_path / "whole" / "mel.npy"), np.load(tmp_path / "whole" / "audio.npy")
    assert m.dtype == np.float32 and a.dtype == np.float64
    assert np.array_equal(m, mel.numpy()) and np.array_equal(a, audio.numpy())
    # over the budget: each array a sorted, seeded sample of its elements, the same on every call
    monkeypatch.setattr(bench, "DUMP_BUDGET", (1 << 16) + 2 * 4000)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), [("mel", mel), ("audio", audio)])
    m1, a1 = np.load(tmp_path / "s1" / "mel.npy"), np.load(tmp_path / "s1" / "audio.npy")
    assert m1.shape == (1000,) and a1.shape == (500,)
    assert np.array_equal(m1, np.load(tmp_path / "s2" / "mel.npy"))
    assert np.array_equal(a1, np.load(tmp_path / "s2" / "audio.npy"))
    idx = torch.randint(0, mel.numel(), (1000,), generator=torch.Generator().manual_seed(bench.DUMP_SEED)).sort().values
    assert np.array_equal(m1, mel.reshape(-1)[idx].numpy())
    total = sum(os.path.getsize(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1"))
    assert total <= bench.DUMP_BUDGET


@pytest.mark.gpu
def test_plain_run_is_the_headline_only(gpu, tmp_path, capsys, monkeypatch):
    """A plain run calls the vocoder warmup + steps times (no settling at
    --settle-ms 0, no event passes, no other line), prints the contract keys,
    and dumps the audio of its last step: the same bits as a direct call on
    the same seeded input and weights."""
    from models.tts_model import SimpleVocoder
    calls = [0]
    voc0 = SimpleVocoder.forward

    def counted(self, mel):
        calls[0] += 1
        return voc0(self, mel)

    monkeypatch.setattr(SimpleVocoder, "forward", counted)
    bench.run(bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "2", "--settle-ms", "0",
                                "--dump-outputs", str(tmp_path)]))
    monkeypatch.undo()
    assert calls[0] == 5
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == bench.METRIC and d["unit"] == "audio samples/s" and d["higher_is_better"] is True
    assert d["steps"] == 3 and d["warmup"] == 2 and d["full"] is False and d["dtype"] == bench.VOC_PATHS[2][0]
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(32 * 32000 / (d["ms_per_step"] * 1e-3), rel=1e-3)
    for k in ("roofline", "vocoder_kernels", "pipeline", "vocoder_exact_f32", "s2_b64_sharded", "cpu_baseline"):
        assert k not in d
    assert os.listdir(tmp_path) == ["audio.npy"]
    audio = np.load(tmp_path / "audio.npy")
    assert audio.dtype == np.float32 and audio.shape == (32, 1, 32000)
    m = bench.fixture_model(bench.STAGE1, gpu)
    mel = torch.randn(32, 64, 500, generator=torch.Generator().manual_seed(1000)).to(gpu)
    assert np.array_equal(audio, m.vocoder(mel).cpu().numpy())
