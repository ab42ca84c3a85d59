#!/usr/bin/env python3
"""Time corpus featurization on the GPU with HIP events.

    python tools/time_features.py [--utterances 256] [--min-seconds 1] [--max-seconds 10] [--repeats 9]

A seeded corpus of PCM16 utterances, lengths uniform between the two bounds at
22050 Hz, resident on the device.  Two ways to its features are timed in turn,
(a), (b), (a), (b), ... in one process:

  (a) one Dsp.mel_features_ragged call over the packed int16 corpus (PCM
      conversion, peak normalisation, features, padded batch);
  (b) a loop of Dsp.mel_spectrogram, one utterance per call, over the
      float32 signals normalised beforehand on the host - the only correct
      path before the ragged call existed, without its host arithmetic and
      without its per-file upload and download.

Before anything is timed the script asserts that (a) and (b) agree bit for
bit on every utterance.  Prints one JSON line: the median, minimum and maximum
milliseconds of --repeats runs of each after --warmup untimed ones, and for (a)
frames per second and seconds of audio per second.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "m2-tts_amd" / "src"))

SR = 22050


def timed_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=256)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--max-seconds", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()

    from m2amd.dsp import get_dsp
    dev = torch.device("cuda", 0)
    d = get_dsp(device=dev)
    rng = np.random.default_rng(args.seed)
    lengths = rng.integers(int(args.min_seconds * SR), int(args.max_seconds * SR) + 1, args.utterances)
    pcm, signals = [], []
    for b, L in enumerate(lengths):
        t = np.arange(L) / SR
        y = (0.4 + 0.5 * rng.random()) * (0.5 * np.sin(2 * np.pi * (110 + 20 * (b % 17)) * t)
                                          + 0.2 * np.sin(2 * np.pi * 3100 * t) + 0.05 * rng.standard_normal(L))
        s = np.clip(np.rint(y * 32767.0), -32768, 32767).astype(np.int16)
        pcm.append(s)
        f = s.astype(np.float32) / np.float32(32768.0)
        signals.append(torch.from_numpy(f / np.max(np.abs(f))).to(dev))
    packed = torch.from_numpy(np.concatenate(pcm)).to(dev)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    T_out = 1 + int(lengths.max()) // d.hop
    out = torch.empty(args.utterances, d.n_mels, T_out, device=dev)

    def ragged():
        return d.mel_features_ragged(packed, offsets=offsets, out=out)

    def loop():
        return [d.mel_spectrogram(y) for y in signals]

    mel, frames = ragged()
    singles = loop()
    frames = frames.tolist()
    for b, m in enumerate(singles):
        assert frames[b] == m.shape[2] and torch.equal(mel[b, :, :frames[b]].view(torch.int32), m[0].view(torch.int32)), b
        assert not mel[b, :, frames[b]:].any(), b
    for _ in range(args.warmup):
        ragged()
        loop()
    torch.cuda.synchronize()
    ms_a, ms_b = [], []
    for _ in range(args.repeats):
        ms_a.append(timed_once(ragged))
        ms_b.append(timed_once(loop))
    a, b = spread(ms_a), spread(ms_b)
    total_frames, seconds = int(sum(frames)), float(lengths.sum()) / SR
    result = {"utterances": args.utterances, "samples": int(lengths.sum()), "audio_seconds": seconds,
              "frames": total_frames, "repeats": args.repeats, "bit_identical": True,
              "ragged_call": a, "per_utterance_loop": b, "speedup_of_medians": b["median_ms"] / a["median_ms"],
              "ragged_frames_per_s": total_frames / (a["median_ms"] * 1e-3),
              "ragged_audio_seconds_per_s": seconds / (a["median_ms"] * 1e-3)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
