"""The configurations and signals shared by the audio-DSP edge tests
(tests/test_audio_oracle.py on the host, tests/test_gpu_dsp_edges.py on the
GPU).  TEST INFRASTRUCTURE ONLY, like audio_oracle.py."""
from __future__ import annotations

import numpy as np

import audio_oracle as ao

# (sample_rate, n_fft, hop, win_length, n_mels, fmin, fmax); tests speak of them as 1..6
CONFIGS = [
    (22050, 1024, 256, 1024, 80, 0, 11025),
    (22050, 512, 128, 512, 40, 0, 11025),
    (22050, 2048, 512, 2048, 80, 0, 11025),
    (22050, 1024, 200, 800, 64, 50, 8000),
    (16000, 512, 160, 400, 40, 20, 7600),
    (22050, 2048, 300, 1200, 80, 0, 11025),
]
# hop > win_length: frames leave gaps, so output samples INSIDE the trimmed
# signal have a window-sum-square of exactly 0 (at configuration 4 the zero
# flanks fall in the centre padding only, see tests/test_gpu_dsp_edges.py)
GAP_CONFIG = (22050, 512, 256, 200, 40, 0, 11025)


def config_id(cfg) -> str:
    return "sr%d-n%d-h%d-w%d-m%d-f%d-%d" % cfg


def tone_noise(n: int, seed: int = 0, scale: float = 1.0) -> np.ndarray:
    """The signal of tests/test_gpu_audio_features.py: two tones and a noise floor."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 22050.0
    s = 0.5 * np.sin(2 * np.pi * 220 * t) + 0.25 * np.sin(2 * np.pi * 3100 * t) + 0.05 * rng.standard_normal(n)
    return (scale * s).astype(np.float32)


def two_tone(n: int, scale: float = 1.0) -> np.ndarray:
    """The same two tones without the noise floor."""
    t = np.arange(n) / 22050.0
    return (scale * (0.5 * np.sin(2 * np.pi * 220 * t) + 0.25 * np.sin(2 * np.pi * 3100 * t))).astype(np.float32)


def stft_lengths(cfg):
    _, n_fft, hop = cfg[:3]
    return [1, hop - 1, hop, hop + 1, n_fft // 2 - 1, n_fft // 2 + 1, n_fft - 1, n_fft + 1, 3 * n_fft + 7]


# name -> which clamp of power_to_db the case is there for (None: neither)
MEL_SIGNALS = {
    "tone_noise": None,
    "silence_then_tones": "floor",
    "silence_then_tones_1e-4": "amin",
    "quiet_then_loud": None,
    "one_frame": None,
    "one_sample": None,
}


def mel_signal(name: str, cfg) -> np.ndarray:
    _, n_fft, hop = cfg[:3]
    if name == "tone_noise":
        return tone_noise(5000, 2)
    if name in ("silence_then_tones", "silence_then_tones_1e-4"):
        y = np.concatenate([np.zeros(3 * n_fft, np.float32), two_tone(3 * n_fft)])
        return y if name == "silence_then_tones" else (y * np.float32(1e-4)).astype(np.float32)
    if name == "quiet_then_loud":
        y = two_tone(6 * n_fft)
        y[:3 * n_fft] *= np.float32(1e-4)
        return y
    if name == "one_frame":
        return tone_noise(hop - 1, 6)
    if name == "one_sample":
        return tone_noise(hop, 7)[-1:]
    raise KeyError(name)


def mel_reference(y: np.ndarray, cfg, dtype=np.float64):
    """(mel power, dB, normalised features) of the oracle at one precision."""
    sr, n_fft, hop, win, n_mels, fmin, fmax = cfg
    P = ao.mel_power(y, sr, n_fft, hop, win, n_mels, fmin, fmax, dtype=dtype)
    db = ao.power_to_db(P, dtype)
    return P, db, ao.normalise_db(db)


def mel_bound(y: np.ndarray, cfg, tol: float = 1e-3):
    """The bound of the GPU features against the float64 reference: the
    project's 1e-3 max-abs; where the float32 restatement (an implementation
    of the same arithmetic the kernel is allowed) is itself further than 1e-4
    from float64, ten times that distance.  -> (bound, that distance)."""
    d = float(np.abs(mel_reference(y, cfg, np.float32)[2].astype(np.float64) - mel_reference(y, cfg)[2]).max())
    return (tol if not d > 1e-4 else 10.0 * d), d


def griffin_inputs(cfg, T_from: int, seed: int, B: int = 2):
    """Magnitudes [B, F, T] float32 (of tone_noise signals at B different
    scales) and unit start phases [B, F, T] complex64 for T = 1 + T_from // hop."""
    _, n_fft, hop, win = cfg[:4]
    rng = np.random.default_rng(seed)
    S = np.stack([np.abs(ao.stft(tone_noise(T_from, seed + b, 1.0 + 2.5 * b), n_fft, hop, win)).astype(np.float32)
                  for b in range(B)])
    ang = np.exp(2j * np.pi * rng.random(S.shape)).astype(np.complex64)
    return S, ang
