#!/usr/bin/env python3
"""Generate tests/golden/eval_reference.json from the reference's own
src/evaluation/metrics.py.

Run on the CPU, in the container that holds the read-only reference (it does
not exist on the GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_eval_golden.py

The reference imports librosa, which is not installed here.  A module of our
own named ``librosa`` is placed in sys.modules first; it supplies only the four
calls metrics.py makes, restated from librosa 0.10's published algorithms:
  stft                        oracle/audio_oracle.py's stft
  feature.mfcc(S=, n_mfcc=)   scipy.fftpack.dct(S, axis=-2, type=2, norm='ortho')[:n_mfcc]
  feature.spectral_centroid   sum_k f_k S_k / sum_k S_k (util.normalize(norm=1):
                              a column whose sum is below tiny divides by 1)
  feature.spectral_bandwidth  (sum_k S_k / sum S (f_k - centroid)^2)^(1/2)
So the reference's code produces the expected dicts: formulas, key names,
averaging and the report text are the reference's; only the librosa calls are
restated, and their parity with librosa proper is UNPINNED.

Each case is evaluated three times by the same reference code:
  ref  float32 inputs, the stub's stft as above (float64 FFT rounded to
       complex64): the reference's result as a user would get it;
  f64  float64 inputs and a complex128 STFT of the same float32 windowed
       frames: the formulas in double - what the GPU result is compared with;
  f32  float32 inputs and scipy.fft.rfft on the float32 frames: a true
       single-precision evaluation.  |f32 - f64| / |f64| is the recorded
       spread, from which the tests take their tolerance.
Only data is written (inputs are named by seed or fixture in eval_cases.py).
"""
import json
import os
import sys
import types
from pathlib import Path

import numpy as np
import scipy.fft
import scipy.fftpack
import torch

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
REF_SRC = Path("/root/reference/src")
sys.path.insert(0, str(REPO / "oracle"))
sys.path.insert(0, str(HERE))

import audio_oracle as ao  # noqa: E402
import eval_cases as ec  # noqa: E402

MODE = "ref"
MAG_RANGE = [np.inf, 0.0]  # smallest / largest STFT magnitude seen over every call


def _frames(y, n_fft, hop):
    win = ao.hann_periodic(n_fft)
    yp = np.pad(np.asarray(y).astype(np.float32), n_fft // 2, mode="constant")
    n = 1 + (len(yp) - n_fft) // hop
    idx = np.arange(n_fft)[None, :] + hop * np.arange(n)[:, None]
    return yp[idx] * win[None, :]  # float32, as the oracle's stft and the GPU's frame loader


def stft(y, n_fft=2048, hop_length=None, **_):
    hop = hop_length if hop_length is not None else n_fft // 4
    if MODE == "ref":
        S = ao.stft(np.asarray(y), n_fft, hop, n_fft)
    elif MODE == "f64":
        S = np.fft.rfft(_frames(y, n_fft, hop).astype(np.float64), axis=1).T
        assert S.dtype == np.complex128
    else:
        S = scipy.fft.rfft(_frames(y, n_fft, hop), axis=1).T
        assert S.dtype == np.complex64
    mag = np.abs(S)
    MAG_RANGE[0], MAG_RANGE[1] = min(MAG_RANGE[0], float(mag.min())), max(MAG_RANGE[1], float(mag.max()))
    return S


def _normalize1(S):
    length = np.sum(np.abs(S), axis=-2, keepdims=True)
    length[length < np.finfo(np.float32).tiny] = 1.0
    return S / length


def _freqs(S, sr):
    return np.fft.rfftfreq(2 * (S.shape[-2] - 1), 1.0 / sr)[:, None]


def spectral_centroid(*, S, sr=22050, **_):
    return np.sum(_freqs(S, sr) * _normalize1(S), axis=-2, keepdims=True)


def spectral_bandwidth(*, S, sr=22050, p=2, **_):
    deviation = np.abs(_freqs(S, sr) - spectral_centroid(S=S, sr=sr))
    return np.sum(_normalize1(S) * deviation ** p, axis=-2, keepdims=True) ** (1.0 / p)


def mfcc(*, S, n_mfcc=20, **_):
    return scipy.fftpack.dct(S, axis=-2, type=2, norm="ortho")[..., :n_mfcc, :]


def install_stub():
    lib = types.ModuleType("librosa")
    lib.stft = stft
    lib.feature = types.ModuleType("librosa.feature")
    lib.feature.mfcc, lib.feature.spectral_centroid, lib.feature.spectral_bandwidth = (mfcc, spectral_centroid,
                                                                                       spectral_bandwidth)
    sys.modules["librosa"], sys.modules["librosa.feature"] = lib, lib.feature


def three_ways(fn):
    """fn(dtype) -> dict of floats, under the three modes -> ref / f64 / spread."""
    global MODE
    out = {}
    for MODE, dt in (("ref", np.float32), ("f64", np.float64), ("f32", np.float32)):
        with np.errstate(all="ignore"):
            out[MODE] = {k: float(v) for k, v in fn(dt).items()}
    MODE = "ref"
    spread = {k: (abs(out["f32"][k] - v) / abs(v) if v != 0 else abs(out["f32"][k])) for k, v in out["f64"].items()}
    return {"ref": out["ref"], "f64": out["f64"], "spread": spread}


def main():
    install_stub()
    sys.path.insert(0, str(REF_SRC))
    from evaluation import metrics as ref  # the reference

    def cast(x, dt):
        return None if x is None else np.asarray(x).astype(dt)

    def tens(x, dt):
        return None if x is None else torch.from_numpy(np.asarray(x).astype(dt))

    doc = {"torch": torch.__version__, "numpy": np.__version__, "cases": {}}
    doc["names"] = sorted(n for n in ("compute_mel_distance", "compute_spectral_convergence",
                                      "compute_log_spectral_distance", "compute_mcd", "estimate_mos_score",
                                      "compute_duration_accuracy", "TTSEvaluator", "benchmark_model_performance")
                          if callable(getattr(ref, n)))
    doc["evaluator_methods"] = sorted(n for n in vars(ref.TTSEvaluator) if not n.startswith("_"))

    for name in ec.AUDIO_CASES:
        pred, target = ec.audio_case(name)
        samples = []
        for b in range(pred.shape[0]):
            t = None if target is None else target[b]
            samples.append(three_ways(lambda dt: ref.estimate_mos_score(cast(pred[b], dt), cast(t, dt), ec.SR)))
            if t is not None:  # the stand-alone functions agree with the dict
                L = min(len(pred[b]), len(t))
                assert float(ref.compute_spectral_convergence(pred[b][:L], t[:L])) == \
                    samples[-1]["ref"]["spectral_convergence"]
                assert float(ref.compute_log_spectral_distance(pred[b][:L], t[:L])) == \
                    samples[-1]["ref"]["log_spectral_distance"]
        doc["cases"][name] = {"samples": samples}

    pm, tm, ml = ec.mel_case()
    samples = []
    for b in range(pm.shape[0]):
        n = int(ml[b])

        def mel(dt, b=b, n=n):
            p, t = pm[b, :n].T, tm[b, :, :n]  # evaluate_batch's cut and transpose (metrics.py:244-257)
            d = ref.compute_mel_distance(tens(p, dt), tens(t, dt))
            d["mcd"] = ref.compute_mcd(cast(p, dt), cast(t, dt))
            return d
        samples.append(three_ways(mel))
    doc["cases"]["mel"] = {"samples": samples}

    pd, td = ec.duration_case()
    doc["cases"]["duration"] = {"samples": [
        three_ways(lambda dt, b=b: ref.compute_duration_accuracy(tens(pd[b], dt), tens(td[b], dt)))
        for b in range(pd.shape[0])]}
    assert doc["cases"]["duration"]["samples"][2]["ref"]["duration_correlation"] == 0.0

    b3 = ec.batch3_case()
    ev = ref.TTSEvaluator(ec.SR)
    doc["cases"]["batch3"] = {"samples": [three_ways(lambda dt: ev.evaluate_batch(
        **{k: (torch.from_numpy(v) if k == "mel_lengths" else tens(v, dt)) for k, v in b3.items()}))]}

    doc["dict_keys"] = {
        "compute_mel_distance": list(ref.compute_mel_distance(tens(pm[0].T, np.float32), tens(tm[0], np.float32))),
        "compute_duration_accuracy": list(doc["cases"]["duration"]["samples"][0]["ref"]),
        "estimate_mos_score": list(doc["cases"]["ragged"]["samples"][0]["ref"]),
        "estimate_mos_score_free": list(doc["cases"]["free"]["samples"][0]["ref"]),
        "evaluate_batch": list(doc["cases"]["batch3"]["samples"][0]["ref"]),
    }
    doc["reports"] = {k: {"metrics": m, "report": ev.generate_evaluation_report(dict(m))}
                      for k, m in ec.REPORT_CASES.items()}

    # The condition that keeps ln(|X| + 1e-8) well-conditioned: every STFT bin
    # of every signal above lies in [1e-3, 200].
    assert 1e-3 <= MAG_RANGE[0] and MAG_RANGE[1] <= 200.0, MAG_RANGE
    doc["stft_magnitude_range"] = MAG_RANGE
    (HERE / "eval_reference.json").write_text(json.dumps(doc, indent=1) + "\n")
    worst = {}
    for c in doc["cases"].values():
        for s in c["samples"]:
            for k, v in s["spread"].items():
                worst[k] = max(worst.get(k, 0.0), v)
    for k, v in sorted(worst.items()):
        print(f"{k:28s} {v:.3e}")
    print("stft magnitudes", MAG_RANGE)


if __name__ == "__main__":
    main()
