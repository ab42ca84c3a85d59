"""Inputs of the training-loss cases, by seed (pure numpy).

Shared by make_losses_golden.py, which runs the reference's losses.py on them
and records the results in losses_reference.json, and by the tests that run the
GPU implementation on the same inputs.  Nothing here is stored as an array.

The shapes are the smallest at which the kernels can still go wrong:
  smoke40  the reference's own smoke shape (test_stage2_simple.py:81-86);
           layer lengths 2560/640/160/40/10, 1280/320/80/20/5 and
           640/160/40/10/3: the last strided layer of scale 4 has a k = 41
           window wider than its input of 10.
  edge41   audio 2624: lengths 2624/656/164/41/11, 1312/328/82/21/6 and
           656/164/41/11/3: non-multiples of 4, partial MFMA column tiles on
           every layer (N = 22, 12 and 6 columns on the dense one).
  one      B = 1, audio 1025: the shortest SpectralLoss accepts.
  odd      B = 3, audio 1001, discriminator only: floor pooling drops a sample.
"""
import math

import numpy as np

SR = 22050
WEIGHT_SEED = 1234  # torch.manual_seed(WEIGHT_SEED); CombinedTTSLoss()
N_FFTS = (512, 1024, 2048)
SAMPLES = 256  # recorded values per feature map

#        B  T   M   S  L     mel_lengths  seed
CASES = {
    "smoke40": (2, 40, 80, 9, 2560, (40, 33), 40),
    "edge41": (2, 12, 80, 5, 2624, (12, 7), 41),
    "one": (1, 6, 80, 3, 1025, None, 1),
    "odd": (3, 0, 0, 0, 1001, None, 3),
}
FULL_CASES = ("smoke40", "edge41", "one")  # CombinedTTSLoss runs on these; "odd" is too short for the STFTs
DISC_CASES = tuple(CASES)

# the seven Conv1d of one discriminator: Cin, Cout, k, stride, padding, groups
LAYERS = ((1, 64, 15, 1, 7, 1), (64, 128, 41, 4, 20, 4), (128, 256, 41, 4, 20, 16), (256, 512, 41, 4, 20, 64),
          (512, 1024, 41, 4, 20, 256), (1024, 1024, 5, 1, 2, 1), (1024, 1, 3, 1, 1, 1))
SCALES = (1, 2, 4)


def audio_case(name):
    """(pred, target) float32 [B, 1, L]: tanh of seeded noise plus a tone; pred a perturbed target."""
    B, _, _, _, L, _, seed = CASES[name]
    rng = np.random.default_rng(seed)
    t = np.arange(L) / SR
    tone = np.stack([0.6 * np.sin(2 * np.pi * (220.0 * (b + 1)) * t + b) for b in range(B)])
    pre = 0.5 * rng.standard_normal((B, L)) + tone
    target = np.tanh(pre)
    pred = np.tanh(pre + 0.15 * rng.standard_normal((B, L)))
    return pred[:, None].astype(np.float32), target[:, None].astype(np.float32)


def loss_case(name):
    """The keyword arguments of CombinedTTSLoss.forward as numpy arrays (mel_lengths may be None)."""
    B, T, M, S, L, lengths, seed = CASES[name]
    rng = np.random.default_rng(1000 + seed)
    pred, target = audio_case(name)
    mel_target = rng.standard_normal((B, M, T)).astype(np.float32)
    mel_pred = (mel_target.transpose(0, 2, 1) + 0.3 * rng.standard_normal((B, T, M))).astype(np.float32)
    dur_target = (rng.random((B, S)) * 4 + 0.5).astype(np.float32)
    dur_pred = (dur_target + 0.4 * rng.standard_normal((B, S))).astype(np.float32)
    return {"mel_pred": np.ascontiguousarray(mel_pred), "mel_target": mel_target, "duration_pred": dur_pred,
            "duration_target": dur_target, "audio_pred": pred, "audio_target": target,
            "mel_lengths": None if lengths is None else np.array(lengths, dtype=np.int64)}


def sample_indices(scale_index, layer, numel):
    """The SAMPLES flat indices of feature map (scale, layer) whose values are recorded."""
    return np.random.default_rng(7000 + 10 * scale_index + layer).integers(0, numel, SAMPLES)


def layer_lengths(L, scale):
    """Output lengths of the seven layers at one scale for audio of L samples."""
    n, out = L // scale, []
    for _, _, k, stride, pad, _ in LAYERS:
        n = (n + 2 * pad - k) // stride + 1
        out.append(n)
    return out


def symmetric_frames(L, hop):
    """Frames of torch.stft(center=True, pad_mode='reflect') that are symmetric about their
    centre: frame 0 (centred on sample 0) and, when L - 1 is a multiple of the hop, the last
    one (centred on sample L - 1)."""
    return [0] + ([(L - 1) // hop] if (L - 1) % hop == 0 and L > 1 else [])


def fingerprint(values):
    """(sum, sum of squares) of a float32 array, exactly rounded (math.fsum: the
    squares of float32 values are exact in float64), so no summation order enters."""
    v = np.asarray(values, dtype=np.float32).astype(np.float64).reshape(-1)
    return math.fsum(v.tolist()), math.fsum((v * v).tolist())


def stft_loss(P, T):
    """SpectralLoss.stft_loss's formula on two complex spectra (numpy, their own
    precision): mean | |P| - |T| | + 0.1 mean |angle P - angle T|."""
    return float(np.mean(np.abs(np.abs(P) - np.abs(T))) + 0.1 * np.mean(np.abs(np.angle(P) - np.angle(T))))


EARLY_STOPPING = {"patience": 3, "min_delta": 0.1,
                  "sequence": [5.0, 4.0, 3.95, 3.91, 3.5, 3.5, 3.45, 3.41, 3.39, 1.0, 1.0]}
