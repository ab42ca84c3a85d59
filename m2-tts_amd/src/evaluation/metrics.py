"""Evaluation metrics for TTS quality (reference src/evaluation/metrics.py).

Same names, signatures, return types and dict keys as the reference, computed
on the GPU: the reference runs librosa and numpy per utterance on the CPU;
here the sums come from the m2_eval_* kernels (m2amd.dsp: a paired STFT that
never stores a spectrum, time-domain statistics, pair statistics, the MCD
dot products), batched over utterances, and only the scalar finishing (log10,
clips, the MOS weights, the correlation) happens on the host, in float64.

Inputs may be torch tensors or numpy arrays; numpy is uploaded.  Like the rest
of the product path there is no CPU fallback: without a ROCm GPU every metric
raises RuntimeError (the module itself imports anywhere).

``TTSEvaluator.evaluate_batch`` is the fast path: one set of launches for the
whole batch and one device-to-host copy of the [B, K] rows.
``estimate_mos_score`` is the reference's heuristic, reproduced as defined.
"""
from __future__ import annotations

import logging
from typing import Dict, List

import numpy as np
import torch

logger = logging.getLogger(__name__)

N_FFT, HOP = 1024, 256  # the reference's librosa.stft(n_fft=1024, hop_length=256) calls


def _on_gpu(x) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if t.device.type != "cuda":
        if not torch.cuda.is_available():
            raise RuntimeError("m2-tts_amd evaluation metrics run on a ROCm GPU; none is visible (no CPU path)")
        t = t.to("cuda")
    return t.detach().float()


def _dsp(sample_rate: int, device):
    from m2amd.dsp import get_dsp
    return get_dsp(sample_rate, N_FFT, HOP, N_FFT, device=device)


def _columns(kind: str, rows: np.ndarray) -> Dict[str, np.ndarray]:
    from m2amd.dsp import eval_columns
    return {name: rows[:, i] for i, name in enumerate(eval_columns(kind))}


# ---- host finishing: [B] float64 vectors from the kernels' sums -----------------

def _mel_metrics(c: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    with np.errstate(divide="ignore", invalid="ignore"):
        l1, l2 = c["abs_diff"] / c["count"], c["sq_diff"] / c["count"]
    return {"mel_l1_distance": l1, "mel_l2_distance": l2, "mel_combined_distance": l1 + np.sqrt(l2)}


def _duration_metrics(c: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    with np.errstate(divide="ignore", invalid="ignore"):
        l1, l2 = c["abs_diff"] / c["count"], c["sq_diff"] / c["count"]
        corr = c["cen_pt"] / np.sqrt(c["cen_pp"] * c["cen_tt"])
    corr = np.where(np.isnan(corr) | (c["count"] <= 1), 0.0, np.clip(corr, -1.0, 1.0))
    return {"duration_l1_loss": l1, "duration_l2_loss": l2, "duration_correlation": corr}


def _audio_metrics(c: Dict[str, np.ndarray], has_target: bool) -> Dict[str, np.ndarray]:
    m: Dict[str, np.ndarray] = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        if has_target:
            snr = 10.0 * np.log10((c["target_sq"] / c["pair_len"]) / (c["noise_sq"] / c["pair_len"] + 1e-8))
            spec_conv = np.sqrt(c["spec_err_sq"]) / (np.sqrt(c["spec_ref_sq"]) + 1e-8)
            lsd = np.sqrt(c["log_spec_sq"] / c["pair_bins"])
            m["snr_db"], m["spectral_convergence"], m["log_spectral_distance"] = snr, spec_conv, lsd
        m["rms_energy"] = np.sqrt(c["pred_sq"] / c["pred_len"])
        m["zero_crossing_rate"] = c["sign_changes"] / (c["pred_len"] - 1.0)
        m["spectral_centroid"] = c["centroid_sum"] / c["pred_frames"]
        m["spectral_bandwidth"] = c["bandwidth_sum"] / c["pred_frames"]
    if has_target:
        score = (0.4 * np.clip((snr + 20.0) / 40.0, 0, 1) + 0.3 * np.clip(1.0 - spec_conv, 0, 1)
                 + 0.3 * np.clip(1.0 - lsd / 5.0, 0, 1))
    else:
        score = 0.5 * np.clip(m["rms_energy"] * 10.0, 0, 1) + 0.5 * np.clip(m["spectral_centroid"] / 3000.0, 0, 1)
    m["estimated_mos"] = np.clip(1.0 + 4.0 * score, 1.0, 5.0)
    return m


def _first(metrics: Dict[str, np.ndarray]) -> Dict[str, float]:
    return {k: float(v[0]) for k, v in metrics.items()}


def _pair_rows(pred, target) -> Dict[str, np.ndarray]:
    """Pair statistics of two equally shaped arrays taken as one utterance."""
    from m2amd.dsp import pair_stats
    p, t = _on_gpu(pred), _on_gpu(target)
    if p.device != t.device:
        t = t.to(p.device)
    p, t = torch.broadcast_tensors(p, t)
    rows = pair_stats(p.reshape(1, 1, -1), t.reshape(1, 1, -1))
    return _columns("pair", rows.cpu().numpy())


# ---- the reference's functions ---------------------------------------------------

def compute_mel_distance(pred_mel, target_mel) -> Dict[str, float]:
    """Mel-spectrogram distance: mean |p - t|, mean (p - t)^2 and l1 + sqrt(l2)."""
    return _first(_mel_metrics(_pair_rows(pred_mel, target_mel)))


def _audio_rows(pred_audio, target_audio, sample_rate: int) -> Dict[str, np.ndarray]:
    p = _on_gpu(pred_audio)
    t = None if target_audio is None else _on_gpu(target_audio).to(p.device)
    return _columns("audio", _dsp(sample_rate, p.device).eval_audio(p, t).cpu().numpy())


def compute_spectral_convergence(pred_audio, target_audio) -> float:
    """||  |STFT(target)| - |STFT(pred)|  ||_F / (|| |STFT(target)| ||_F + 1e-8)."""
    return _first(_audio_metrics(_audio_rows(pred_audio, target_audio, 22050), True))["spectral_convergence"]


def compute_log_spectral_distance(pred_audio, target_audio) -> float:
    """sqrt(mean (ln(|STFT(pred)| + 1e-8) - ln(|STFT(target)| + 1e-8))^2)."""
    return _first(_audio_metrics(_audio_rows(pred_audio, target_audio, 22050), True))["log_spectral_distance"]


def compute_mcd(pred_mel, target_mel) -> float:
    """Mel-cepstral distortion of two [n_mels, frames] spectrograms, cut to the
    shorter one: mean over frames of the distance of their first 13 DCT-II
    coefficients (librosa.feature.mfcc(S=., n_mfcc=13))."""
    from m2amd.dsp import mcd
    p, t = _on_gpu(pred_mel), _on_gpu(target_mel)
    c = _columns("mcd", mcd(p.reshape(1, *p.shape[-2:]), t.to(p.device).reshape(1, *t.shape[-2:])).cpu().numpy())
    with np.errstate(divide="ignore", invalid="ignore"):
        return float((c["mcd_sum"] / c["frames"])[0])


def estimate_mos_score(pred_audio, target_audio=None, sample_rate: int = 22050) -> Dict[str, float]:
    """The reference's MOS heuristic from audio quality metrics (a rough
    approximation: a real MOS needs listeners)."""
    return _first(_audio_metrics(_audio_rows(pred_audio, target_audio, sample_rate), target_audio is not None))


def compute_duration_accuracy(pred_durations, target_durations) -> Dict[str, float]:
    """Duration prediction accuracy: L1, L2 and the correlation (0.0 where undefined)."""
    return _first(_duration_metrics(_pair_rows(pred_durations, target_durations)))


class TTSEvaluator:
    """The reference's evaluator: per-sample metrics, batch means and a text report."""

    def __init__(self, sample_rate: int = 22050):
        self.sample_rate = sample_rate

    def _rows(self, pred_mels, target_mels, pred_audios, target_audios, pred_durations, target_durations,
              mel_lengths, transposed: bool) -> Dict[str, np.ndarray]:
        """Per-sample metrics as [B] vectors: every launch covers the batch, one copy to the host."""
        from m2amd.dsp import pair_stats
        tm = _on_gpu(target_mels)
        dev = tm.device
        B = tm.shape[0]
        cols = None
        if mel_lengths is not None:
            ml = mel_lengths if isinstance(mel_lengths, torch.Tensor) else torch.as_tensor(np.asarray(mel_lengths))
            cols = ml.to(dev).reshape(B).clamp(min=0, max=tm.shape[2]).to(torch.int32)
        parts = [("pair", pair_stats(_on_gpu(pred_mels).to(dev), tm, transposed=transposed, cols=cols), _mel_metrics)]
        if pred_audios is not None:
            pa = _on_gpu(pred_audios).to(dev).reshape(B, -1)
            ta = None if target_audios is None else _on_gpu(target_audios).to(dev).reshape(B, -1)
            has_target = ta is not None
            parts.append(("audio", _dsp(self.sample_rate, dev).eval_audio(pa, ta),
                          lambda c: _audio_metrics(c, has_target)))
        if pred_durations is not None and target_durations is not None:
            pd, td = _on_gpu(pred_durations).to(dev).reshape(B, 1, -1), _on_gpu(target_durations).to(dev).reshape(B, 1, -1)
            parts.append(("pair", pair_stats(pd, td), _duration_metrics))
        rows = torch.cat([r for _, r, _ in parts], dim=1).cpu().numpy()
        out: Dict[str, np.ndarray] = {}
        k = 0
        for kind, r, finish in parts:
            out.update(finish(_columns(kind, rows[:, k:k + r.shape[1]])))
            k += r.shape[1]
        return out

    def evaluate_sample(self, pred_mel, target_mel, pred_audio=None, target_audio=None, pred_durations=None,
                        target_durations=None) -> Dict[str, float]:
        """Evaluate a single sample (pred_mel and target_mel in the same layout)."""
        p, t = _on_gpu(pred_mel), _on_gpu(target_mel)
        p, t = torch.broadcast_tensors(p, t.to(p.device))
        rows = self._rows(p.reshape(1, 1, -1), t.reshape(1, 1, -1),
                          None if pred_audio is None else _on_gpu(pred_audio).reshape(1, -1),
                          None if target_audio is None else _on_gpu(target_audio).reshape(1, -1),
                          None if pred_durations is None else _on_gpu(pred_durations).reshape(1, -1),
                          None if target_durations is None else _on_gpu(target_durations).reshape(1, -1),
                          None, False)
        return _first(rows)

    def evaluate_batch(self, pred_mels, target_mels, pred_audios=None, target_audios=None, pred_durations=None,
                       target_durations=None, mel_lengths=None) -> Dict[str, float]:
        """Evaluate a batch: pred_mels [B, T, M] (the model's layout) against
        target_mels [B, M, T], each cut to mel_lengths[b] frames when given;
        audios [B, L] (or [B, 1, L]); durations [B, S].  The per-sample
        metrics averaged over the batch."""
        tm = target_mels
        if tm.ndim != 3 or pred_mels.ndim != 3 or tuple(pred_mels.shape) != (tm.shape[0], tm.shape[2], tm.shape[1]):
            raise ValueError(f"evaluate_batch: pred_mels {tuple(pred_mels.shape)} must be [B, T, M] for "
                             f"target_mels {tuple(tm.shape)} [B, M, T]")
        if tm.shape[0] == 0:
            return {}
        rows = self._rows(pred_mels, target_mels, pred_audios, target_audios, pred_durations, target_durations,
                          mel_lengths, True)
        return {k: np.mean(v) for k, v in rows.items()}

    def generate_evaluation_report(self, metrics: Dict[str, float]) -> str:
        """The metrics as text: the MOS line with its quality band, then every metric by name."""
        lines = ["TTS Model Evaluation Report", "=" * 40, ""]
        if "estimated_mos" in metrics:
            mos = metrics["estimated_mos"]
            bands = ((4.0, "Excellent"), (3.5, "Good"), (3.0, "Fair"))
            quality = next((name for floor, name in bands if mos >= floor), "Poor")
            lines += [f"Overall Quality (Est. MOS): {mos:.2f}/5.0", f"Quality Rating: {quality}", ""]
        lines += ["Detailed Metrics:", "-" * 20]
        for name, value in sorted(metrics.items()):
            lines.append(f"{name}: {value:.4f}" if isinstance(value, float) else f"{name}: {value}")
        return "\n".join(lines) + "\n"


def benchmark_model_performance(model, dataloader, device: torch.device, num_samples: int = 100) -> Dict[str, float]:
    """Score a model over a dataloader of batch dicts (phoneme_ids, text_lengths,
    durations, mel_specs [B, M, T], mel_lengths): teacher-forced forward passes
    until ``num_samples`` utterances are covered, each batch through
    TTSEvaluator.evaluate_batch; returns the mean of the batch results."""
    model.eval()
    evaluator = TTSEvaluator()
    per_batch: List[Dict[str, float]] = []
    seen = 0
    logger.info(f"scoring up to {num_samples} utterances")
    with torch.no_grad():
        for batch in dataloader:
            if seen >= num_samples:
                break
            batch.update({k: v.to(device) for k, v in batch.items() if isinstance(v, torch.Tensor)})
            out = model(phoneme_ids=batch["phoneme_ids"], phoneme_lengths=batch["text_lengths"],
                        target_durations=batch["durations"], max_target_length=batch["mel_specs"].size(2))
            per_batch.append(evaluator.evaluate_batch(
                pred_mels=out["mel_output"], target_mels=batch["mel_specs"], pred_durations=out["duration_pred"],
                target_durations=batch["durations"], mel_lengths=batch["mel_lengths"]))
            seen += batch["phoneme_ids"].size(0)
    if not per_batch:
        return {}
    return {k: np.mean([m[k] for m in per_batch if k in m]) for k in per_batch[0]}
