"""Inputs of the evaluation-metric cases, by seed or fixture name (pure numpy).

Shared by make_eval_golden.py, which runs the reference's metrics on them and
records the results in eval_reference.json, and by the tests that run the GPU
implementation on the same inputs.  Nothing here is stored as an array.
"""
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
SR = 22050
RAGGED_L = 3 * 1024 + 7

AUDIO_CASES = ("gold", "ragged", "short", "unequal", "free")


def _s1_small():
    return np.load(HERE / "s1_small.npz", allow_pickle=False)


def _ragged(seed=1, n=RAGGED_L):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    target = (0.5 * np.sin(2 * np.pi * 220 * t) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    pred = (0.9 * target + 0.02 * rng.standard_normal(n)).astype(np.float32)
    return pred, target


def _gold():
    target = _s1_small()["audio"][:, 0].astype(np.float32)  # [2, 7680]
    noise = np.random.default_rng(0).standard_normal(target.shape)
    return (target + 0.01 * noise).astype(np.float32), target


def audio_case(name):
    """(pred [B, Lp] float32, target [B, Lt] float32 or None)."""
    if name == "gold":
        return _gold()
    pred, target = _ragged()
    if name == "ragged":
        return pred[None], target[None]
    if name == "short":
        return pred[None, :300], target[None, :300]
    if name == "unequal":
        return pred[None], target[None, :RAGGED_L - 100]
    if name == "free":
        return pred[None], None
    raise KeyError(name)


def mel_case():
    """pred [2, T, M] (the model's layout: the s1_small mel), target [2, M, T]
    (perturbed, transposed), mel_lengths [2] with one utterance shorter than T."""
    pred = _s1_small()["mel"].astype(np.float32)
    noise = np.random.default_rng(3).standard_normal(pred.shape)
    target = np.ascontiguousarray((pred + 0.05 * noise).astype(np.float32).transpose(0, 2, 1))
    return pred, target, np.array([pred.shape[1], pred.shape[1] - 7], dtype=np.int64)


def duration_case():
    """pred, target [3, 12] float32; the last target row is constant."""
    rng = np.random.default_rng(4)
    target = rng.integers(1, 9, (3, 12)).astype(np.float32)
    pred = (target + 0.5 * rng.standard_normal(target.shape)).astype(np.float32)
    target[2] = 5.0
    return pred, target


def batch3_case():
    """evaluate_batch's arguments for a batch of three: audio rows `ragged`, the
    first gold utterance and a second ragged draw, all cut to Lp = RAGGED_L with
    targets 100 samples shorter (the `unequal` shape); mels, durations and
    mel_lengths from mel_case / duration_case (mel rows 0, 1, 0)."""
    rp, rt = _ragged()
    gp, gt = _gold()
    qp, qt = _ragged(seed=7)
    pred_audios = np.stack([rp, gp[0, :RAGGED_L], qp])
    target_audios = np.stack([rt, gt[0, :RAGGED_L], qt])[:, :RAGGED_L - 100]
    pm, tm, _ = mel_case()
    noise = np.random.default_rng(5).standard_normal(tm[0].shape).astype(np.float32)
    pred_mels = np.stack([pm[0], pm[1], pm[0]])
    target_mels = np.stack([tm[0], tm[1], (tm[0] + 0.1 * noise).astype(np.float32)])
    pd, td = duration_case()
    T = pm.shape[1]
    return dict(pred_mels=pred_mels, target_mels=target_mels, pred_audios=pred_audios, target_audios=target_audios,
                pred_durations=pd, target_durations=td, mel_lengths=np.array([T, T - 7, T - 30], dtype=np.int64))


# generate_evaluation_report inputs: one per quality band, floats and a non-float value
REPORT_CASES = {
    "excellent": {"estimated_mos": 4.25, "snr_db": 18.123456, "mel_l1_distance": 0.05, "samples": 12},
    "good": {"estimated_mos": 3.5, "log_spectral_distance": 0.91, "rms_energy": 0.1234},
    "fair": {"estimated_mos": 3.25, "spectral_centroid": 1830.55555},
    "poor": {"estimated_mos": 1.0, "zero_crossing_rate": 0.0},
    "no_mos": {"mel_l2_distance": 0.001, "duration_correlation": -0.25},
}
