"""GPU: the drop-in evaluation.metrics module (reference src/evaluation/metrics.py)
against the reference's own code, recorded in tests/golden/eval_reference.json
by tests/golden/make_eval_golden.py.

librosa is not installed here.  The generator runs the reference's metrics.py
with a module of our own in librosa's place that restates the four librosa
calls it makes (stft from oracle/audio_oracle.py, feature.mfcc via
scipy.fftpack.dct, spectral_centroid, spectral_bandwidth), so formulas, keys,
averaging and report text are pinned to the reference itself, while parity of
those four restatements with librosa proper is UNPINNED.

Every metric is compared, relative, with the float64 evaluation of the
reference's formulas in the JSON.  The bar is 32 x max(s, 2^-24), s being the
largest recorded relative spread, over the cases, of a true single-precision
evaluation (scipy.fft.rfft on float32 frames, float32 arithmetic) from the
float64 one; 32 is the margin the STFT test gives fp32 rounding
(test_gpu_audio_features.py:40).  The bar never comes from the GPU's output.
Recorded spreads (make_eval_golden.py prints them) and the bars they give:

  metric                  spread    bar        metric                 spread    bar
  snr_db                  5.1e-08   1.9e-06    mel_l1_distance        1.2e-07   3.9e-06
  spectral_convergence    2.5e-07   8.1e-06    mel_l2_distance        3.0e-08   1.9e-06
  log_spectral_distance   2.8e-07   9.0e-06    mel_combined_distance  6.2e-08   2.0e-06
  rms_energy              6.1e-08   1.9e-06    mcd                    2.1e-07   6.8e-06
  zero_crossing_rate      3.4e-08   1.9e-06    duration_l1_loss       8.2e-08   2.6e-06
  spectral_centroid       5.6e-08   1.9e-06    duration_l2_loss       2.3e-08   1.9e-06
  spectral_bandwidth      3.4e-08   1.9e-06    duration_correlation   0         1.9e-06
  estimated_mos           5.5e-08   1.9e-06

The inputs keep every STFT bin of both signals in [1e-3, 200] (the generator
asserts it; 3.0e-3 .. 125 here), so ln(|X| + 1e-8) is well-conditioned and the
log spectral distance cannot hide a kernel error behind ill-conditioning.
"""
import json
import sys

import numpy as np
import pytest
import scipy.fft
import torch

from conftest import GOLDEN, golden, golden_state

sys.path.insert(0, str(GOLDEN))
import eval_cases as ec  # noqa: E402

pytestmark = pytest.mark.gpu

REF = json.loads((GOLDEN / "eval_reference.json").read_text())


def _bar(metric):
    s = max(smp["spread"][metric] for c in REF["cases"].values() for smp in c["samples"] if metric in smp["spread"])
    return 32.0 * max(s, 2.0 ** -24)


def _check(got, sample, what):
    want = sample["f64"]
    assert list(got) == list(sample["ref"]), what
    for k, w in want.items():
        err = abs(got[k] - w) / abs(w) if w != 0 else abs(got[k])
        print(f"{what} {k}: got {got[k]!r} f64 {w!r} rel {err:.3e} bar {_bar(k):.3e}")
    for k, w in want.items():
        if w == 0:
            assert got[k] == 0.0, (what, k)
        else:
            assert abs(got[k] - w) <= _bar(k) * abs(w), (what, k, got[k], w)


@pytest.mark.parametrize("case", ec.AUDIO_CASES)
def test_estimate_mos_score_matches_reference(gpu, case):
    from evaluation import metrics
    pred, target = ec.audio_case(case)
    for b, sample in enumerate(REF["cases"][case]["samples"]):
        t = None if target is None else target[b]
        got = metrics.estimate_mos_score(pred[b], t, ec.SR)
        assert all(type(v) is float for v in got.values())
        _check(got, sample, f"{case}[{b}]")
        # exact: the count of sign changes over the un-cut pred
        assert np.float32(got["zero_crossing_rate"]) == np.float32(sample["ref"]["zero_crossing_rate"])
        if t is not None and len(t) == len(pred[b]):
            assert metrics.compute_spectral_convergence(pred[b], t) == got["spectral_convergence"]
            assert metrics.compute_log_spectral_distance(torch.from_numpy(pred[b]), t) == got["log_spectral_distance"]


def test_batched_rows_equal_single_rows_and_repeat_bit_identically(gpu):
    from m2amd.dsp import eval_columns, get_dsp
    d = get_dsp(device=gpu)
    pred, target = (torch.from_numpy(x).to(gpu) for x in ec.audio_case("gold"))
    rows = d.eval_audio(pred, target)
    assert rows.shape == (2, len(eval_columns("audio"))) and rows.dtype == torch.float64 and rows.is_cuda
    assert torch.equal(rows, d.eval_audio(pred, target))
    for b in range(2):
        assert torch.equal(rows[b:b + 1], d.eval_audio(pred[b:b + 1], target[b:b + 1]))
    c = dict(zip(eval_columns("audio"), rows[0].tolist()))
    assert (c["pair_len"], c["pred_len"], c["pred_frames"], c["pair_bins"]) == (7680, 7680, 31, 31 * 513)


def test_evaluate_batch_of_three_matches_reference_mean(gpu):
    from evaluation.metrics import TTSEvaluator
    args = ec.batch3_case()
    ev = TTSEvaluator(ec.SR)
    got = ev.evaluate_batch(**{k: torch.from_numpy(v).to(gpu) for k, v in args.items()})
    assert all(isinstance(v, np.float64) for v in got.values())
    _check(got, REF["cases"]["batch3"]["samples"][0], "batch3")
    again = ev.evaluate_batch(**args)  # numpy inputs are uploaded; two runs give equal bits
    assert again == got


def test_evaluate_sample_is_the_batch_of_one(gpu):
    from evaluation.metrics import TTSEvaluator
    a = ec.batch3_case()
    ev = TTSEvaluator(ec.SR)
    n = int(a["mel_lengths"][1])
    got = ev.evaluate_sample(torch.from_numpy(a["pred_mels"][1, :n].T.copy()), torch.from_numpy(a["target_mels"][1, :, :n].copy()),
                             torch.from_numpy(a["pred_audios"][1:2]), torch.from_numpy(a["target_audios"][1:2]),
                             torch.from_numpy(a["pred_durations"][1]), torch.from_numpy(a["target_durations"][1]))
    one = ev.evaluate_batch(**{k: v[1:2] for k, v in a.items()})
    assert list(got) == list(one) == REF["dict_keys"]["evaluate_batch"]
    for k in got:
        assert type(got[k]) is float
        assert abs(got[k] - one[k]) <= 1e-12 * abs(one[k]), k  # same sums, another summation order over the mel
    free = ev.evaluate_sample(torch.from_numpy(a["pred_mels"][1, :n].T.copy()), torch.from_numpy(a["target_mels"][1, :, :n].copy()),
                              torch.from_numpy(a["pred_audios"][1:2]))
    assert list(free) == REF["dict_keys"]["compute_mel_distance"] + REF["dict_keys"]["estimate_mos_score_free"]


def test_exact_zero_cases(gpu):
    from evaluation import metrics
    z = np.zeros(2000, dtype=np.float32)
    free = metrics.estimate_mos_score(z)
    assert free == {"rms_energy": 0.0, "zero_crossing_rate": 0.0, "spectral_centroid": 0.0, "spectral_bandwidth": 0.0,
                    "estimated_mos": 1.0}
    both = metrics.estimate_mos_score(z, z)
    assert both["log_spectral_distance"] == 0.0 and both["spectral_convergence"] == 0.0
    assert both["snr_db"] == -np.inf and both["rms_energy"] == 0.0


@pytest.mark.parametrize("layout", ["btm", "bmt"])
def test_mel_distance_and_mcd_match_reference(gpu, layout):
    """The s1_small mel [B, T, M] against a perturbed transposed target, one
    utterance shorter than T; pred read transposed in place, or pre-transposed."""
    from m2amd.dsp import eval_columns, mcd, pair_stats
    from evaluation import metrics
    pm, tm, ml = ec.mel_case()
    p = torch.from_numpy(pm).to(gpu)
    t, cols = torch.from_numpy(tm).to(gpu), torch.from_numpy(ml).to(gpu)
    if layout == "bmt":
        p = p.transpose(1, 2).contiguous()
    stats = pair_stats(p, t, transposed=layout == "btm", cols=cols).cpu().numpy()
    dist = mcd(p, t, transposed=layout == "btm", cols=cols).cpu().numpy()
    for b, sample in enumerate(REF["cases"]["mel"]["samples"]):
        got = {k: float(v[0]) for k, v in metrics._mel_metrics(
            {c: stats[b:b + 1, i] for i, c in enumerate(eval_columns("pair"))}).items()}
        assert dist[b, 1] == ml[b] and stats[b, 7] == ml[b] * pm.shape[2]
        got["mcd"] = float(dist[b, 0] / dist[b, 1])
        _check(got, sample, f"mel {layout}[{b}]")
        # the reference-shaped entry points on the cut utterance, numpy in
        n = int(ml[b])
        alone = metrics.compute_mel_distance(pm[b, :n].T, tm[b, :, :n])
        alone["mcd"] = metrics.compute_mcd(pm[b, :n].T, tm[b, :, :n + 3 if n + 3 <= tm.shape[2] else n])
        _check(alone, sample, f"mel alone[{b}]")


def test_duration_accuracy_matches_reference(gpu):
    from evaluation import metrics
    pd, td = ec.duration_case()
    for b, sample in enumerate(REF["cases"]["duration"]["samples"]):
        _check(metrics.compute_duration_accuracy(torch.from_numpy(pd[b]).to(gpu), torch.from_numpy(td[b])), sample,
               f"duration[{b}]")
    const = metrics.compute_duration_accuracy(pd[2], td[2])
    assert const["duration_correlation"] == 0.0  # a constant row: the reference maps NaN to 0.0
    assert metrics.compute_duration_accuracy(np.float32([3.0]), np.float32([4.0])) == {
        "duration_l1_loss": 1.0, "duration_l2_loss": 1.0, "duration_correlation": 0.0}


def _host_spectral(pred, target, n_fft, hop, sr, fft, dt):
    """numpy restatement of the four spectral metrics for one utterance; fft / dt choose the precision."""
    win = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)).astype(np.float32)

    def mags(y):
        yp = np.pad(y.astype(np.float32), n_fft // 2)
        idx = np.arange(n_fft)[None, :] + hop * np.arange(1 + len(y) // hop)[:, None]
        return np.abs(fft((yp[idx] * win[None, :]).astype(dt), axis=1)).astype(dt)

    P, T = mags(pred), mags(target)
    f = (np.arange(n_fft // 2 + 1) * (sr / n_fft))[None, :]
    cen = (f * (P / P.sum(1, keepdims=True))).sum(1, keepdims=True)
    bw = np.sqrt(((P / P.sum(1, keepdims=True)) * (f - cen) ** 2).sum(1))
    return {"spectral_convergence": float(np.sqrt(((T - P) ** 2).sum()) / (np.sqrt((T ** 2).sum()) + dt(1e-8))),
            "log_spectral_distance": float(np.sqrt(np.mean((np.log(P + dt(1e-8)) - np.log(T + dt(1e-8))) ** 2))),
            "spectral_centroid": float(cen.mean()), "spectral_bandwidth": float(bw.mean())}


@pytest.mark.parametrize("n_fft,hop", [(512, 128), (2048, 512)])
def test_other_fft_sizes_of_the_handle(gpu, n_fft, hop):
    """The 512- and 2048-point instances of the frame kernel (the reference only
    uses 1024), against numpy in float64; the bar is 32 x the spread of a
    single-precision numpy evaluation of the same inputs, computed here."""
    from m2amd.dsp import Dsp, eval_columns
    from evaluation.metrics import _audio_metrics
    pred, target = ec.audio_case("ragged")
    rows = Dsp(ec.SR, n_fft, hop, n_fft, device=gpu).eval_audio(torch.from_numpy(pred).to(gpu),
                                                               torch.from_numpy(target).to(gpu)).cpu().numpy()
    got = _audio_metrics({c: rows[:, i] for i, c in enumerate(eval_columns("audio"))}, True)
    want = _host_spectral(pred[0], target[0], n_fft, hop, ec.SR, np.fft.rfft, np.float64)
    single = _host_spectral(pred[0], target[0], n_fft, hop, ec.SR, scipy.fft.rfft, np.float32)
    for k, w in want.items():
        bar = 32.0 * max(abs(single[k] - w) / abs(w), 2.0 ** -24)
        print(f"n_fft {n_fft} {k}: got {got[k][0]!r} f64 {w!r} rel {abs(got[k][0] - w) / abs(w):.3e} bar {bar:.3e}")
        assert abs(got[k][0] - w) <= bar * abs(w), k


def test_abi_conventions(gpu):
    from m2amd import _lib
    from m2amd.dsp import get_dsp
    lib = _lib.load()
    d = get_dsp(device=gpu)
    x = torch.zeros(2, 3000, device=gpu)
    out = torch.full((2, 13), -1.0, device=gpu, dtype=torch.float64)
    need = lib.m2_eval_audio_workspace_bytes(d.handle, 2, 3000)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    args = (x.data_ptr(), x.data_ptr(), 2, 3000, 3000, out.data_ptr(), ws.data_ptr())
    assert lib.m2_eval_audio(d.handle, *args, 64, None) == -3  # M2_E_WORKSPACE
    assert b"workspace" in lib.m2_last_error()
    assert lib.m2_eval_audio(d.handle, None, None, 2, 3000, 0, out.data_ptr(), ws.data_ptr(), need, None) == -1
    assert lib.m2_eval_audio(None, *args, need, None) == -1
    assert lib.m2_eval_audio(d.handle, x.data_ptr(), x.data_ptr(), 0, 3000, 3000, out.data_ptr(), None, 0, None) == 0
    assert lib.m2_eval_pair_stats(x.data_ptr(), x.data_ptr(), None, 0, 1, 3000, 0, out.data_ptr(), None) == 0
    assert lib.m2_eval_pair_stats(x.data_ptr(), None, None, 2, 1, 3000, 0, out.data_ptr(), None) == -1
    assert lib.m2_eval_mcd(x.data_ptr(), x.data_ptr(), None, None, 2, 30, 100, 100, 0, out.data_ptr(), None) == -1
    assert lib.m2_eval_audio_workspace_bytes(None, 2, 3000) == 0
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())  # nothing was launched
    tbl = torch.zeros(13, 30, device=gpu, dtype=torch.float64)
    assert lib.m2_eval_mcd(x.data_ptr(), x.data_ptr(), None, tbl.data_ptr(), 0, 30, 100, 100, 0, out.data_ptr(),
                           None) == 0
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        d.eval_audio(torch.zeros(1, 3000))


def test_benchmark_model_performance(gpu):
    """Two batches of dicts through the golden stage-1 model, teacher-forced:
    the keys and values of evaluate_batch run by hand on the same outputs,
    averaged over the batches."""
    from evaluation.metrics import TTSEvaluator, benchmark_model_performance
    from models.tts_model import M2TTSModel
    g = golden("s1_small")
    model = M2TTSModel()
    model.load_state_dict(golden_state("s1"))
    model = model.to(gpu).eval()
    ids, lens = torch.from_numpy(g["ids"]), torch.from_numpy(g["lengths"])
    T = 5 * ids.shape[1]
    rng = np.random.default_rng(11)

    def batch(i):
        mel = np.ascontiguousarray(g["mel"].transpose(0, 2, 1)) + 0.1 * rng.standard_normal((2, 64, T))
        return {"phoneme_ids": ids.flip(0) if i else ids, "text_lengths": lens.flip(0) if i else lens,
                "durations": torch.full(ids.shape, 5.0), "mel_specs": torch.from_numpy(mel.astype(np.float32)),
                "mel_lengths": torch.tensor([T, T - 20 - i]), "speaker": ["a", "b"]}

    batches = [batch(0), batch(1)]
    by_hand = []
    ev = TTSEvaluator()
    for b in batches:
        out = model(phoneme_ids=b["phoneme_ids"].to(gpu), phoneme_lengths=b["text_lengths"].to(gpu),
                    target_durations=b["durations"].to(gpu), max_target_length=T)
        by_hand.append(ev.evaluate_batch(pred_mels=out["mel_output"], target_mels=b["mel_specs"],
                                         pred_durations=out["duration_pred"], target_durations=b["durations"],
                                         mel_lengths=b["mel_lengths"]))
    got = benchmark_model_performance(model, [dict(b) for b in batches], gpu, num_samples=100)
    assert list(got) == REF["dict_keys"]["compute_mel_distance"] + REF["dict_keys"]["compute_duration_accuracy"]
    assert not model.training
    for k in got:
        assert got[k] == np.mean([m[k] for m in by_hand]), k
        assert np.isfinite(got[k])
    one = benchmark_model_performance(model, [dict(b) for b in batches], gpu, num_samples=2)
    assert one == by_hand[0]  # stops once num_samples utterances are scored
    assert benchmark_model_performance(model, [], gpu) == {}
