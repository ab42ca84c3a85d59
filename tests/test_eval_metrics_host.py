"""Host-side checks of the drop-in evaluation.metrics module (no GPU): it
imports, carries the reference's public names and dict keys (recorded from the
reference in tests/golden/eval_reference.json by make_eval_golden.py), writes
the reference's report text, refuses to compute without a GPU, and the host
DCT table of the MCD kernel is scipy's orthonormal DCT-II."""
import ctypes
import inspect
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN

REF = json.loads((GOLDEN / "eval_reference.json").read_text())


def test_module_imports_and_has_the_reference_names():
    from evaluation import metrics
    from evaluation.metrics import TTSEvaluator  # noqa: F401  (the import the reference's trainers use)
    assert sorted(n for n in REF["names"] if callable(getattr(metrics, n, None))) == REF["names"]
    methods = sorted(n for n in vars(metrics.TTSEvaluator) if not n.startswith("_"))
    assert methods == REF["evaluator_methods"]
    assert list(inspect.signature(metrics.TTSEvaluator.evaluate_batch).parameters) == [
        "self", "pred_mels", "target_mels", "pred_audios", "target_audios", "pred_durations", "target_durations",
        "mel_lengths"]
    assert list(inspect.signature(metrics.benchmark_model_performance).parameters) == [
        "model", "dataloader", "device", "num_samples"]
    assert inspect.signature(metrics.estimate_mos_score).parameters["sample_rate"].default == 22050


def test_dict_keys_equal_the_reference():
    """The host finishing on rows of ones: same keys in the same order as the reference's dicts."""
    from evaluation import metrics
    from m2amd.dsp import eval_columns

    def ones(kind):
        return {c: np.ones(1) for c in eval_columns(kind)}

    keys = REF["dict_keys"]
    assert list(metrics._mel_metrics(ones("pair"))) == keys["compute_mel_distance"]
    assert list(metrics._duration_metrics(ones("pair"))) == keys["compute_duration_accuracy"]
    assert list(metrics._audio_metrics(ones("audio"), True)) == keys["estimate_mos_score"]
    assert list(metrics._audio_metrics(ones("audio"), False)) == keys["estimate_mos_score_free"]
    assert keys["evaluate_batch"] == (keys["compute_mel_distance"] + keys["estimate_mos_score"]
                                      + keys["compute_duration_accuracy"])


@pytest.mark.parametrize("band", sorted(REF["reports"]))
def test_report_text_equals_the_reference(band):
    from evaluation.metrics import TTSEvaluator
    case = REF["reports"][band]
    assert TTSEvaluator().generate_evaluation_report(dict(case["metrics"])) == case["report"]
    # np.mean's float64 (what evaluate_batch returns) formats like a float
    as_np = {k: (np.float64(v) if isinstance(v, float) else v) for k, v in case["metrics"].items()}
    assert TTSEvaluator().generate_evaluation_report(as_np) == case["report"]


def test_report_covers_the_four_quality_bands():
    ratings = {k: v["report"].split("Quality Rating: ")[1].split("\n")[0] for k, v in REF["reports"].items()
               if "Quality Rating" in v["report"]}
    assert sorted(ratings.values()) == ["Excellent", "Fair", "Good", "Poor"]


def test_no_gpu_is_a_runtime_error(monkeypatch):
    """CPU inputs with no GPU visible: RuntimeError, as everywhere else (no CPU path)."""
    from evaluation import metrics
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    a = np.zeros(2048, dtype=np.float32)
    mel = torch.zeros(1, 8, 64)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        metrics.estimate_mos_score(a, a)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        metrics.compute_spectral_convergence(a, a)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        metrics.compute_mel_distance(mel, mel)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        metrics.compute_mcd(np.zeros((64, 8), np.float32), np.zeros((64, 8), np.float32))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        metrics.compute_duration_accuracy(torch.ones(5), torch.ones(5))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        metrics.TTSEvaluator().evaluate_batch(mel, mel.transpose(1, 2))


@pytest.mark.parametrize("n_mels", [64, 80, 7])
def test_dct_table_is_scipy_orthonormal_dct2(n_mels):
    import scipy.fftpack
    from m2amd import _lib
    lib = _lib.load()
    n = lib.m2_eval_mcd_coefficients()
    assert n == 13
    buf = (ctypes.c_double * (n * n_mels))()
    assert lib.m2_eval_dct_table(n_mels, buf) == 0
    got = np.array(buf).reshape(n, n_mels)
    want = scipy.fftpack.dct(np.eye(n_mels), axis=0, type=2, norm="ortho")[:n]
    if want.shape[0] < n:  # fewer bands than coefficients: mfcc has n_mels rows, the rest are zero
        assert not got[want.shape[0]:].any()
        got = got[:want.shape[0]]
    assert np.abs(got - want).max() <= 1e-14
    assert lib.m2_eval_dct_table(0, buf) == -1 and lib.m2_eval_dct_table(n_mels, None) == -1


def test_column_names():
    from m2amd import _lib
    from m2amd.dsp import eval_columns
    lib = _lib.load()
    assert [lib.m2_eval_column_count(k) for k in (0, 1, 2, 3)] == [13, 11, 2, -1]
    assert eval_columns("audio")[:4] == ("spec_err_sq", "spec_ref_sq", "log_spec_sq", "pair_bins")
    assert eval_columns("mcd") == ("mcd_sum", "frames")
    assert lib.m2_eval_column_name(1, 11) is None and lib.m2_eval_column_name(9, 0) is None
    assert len(set(eval_columns("audio"))) == 13 and len(set(eval_columns("pair"))) == 11
