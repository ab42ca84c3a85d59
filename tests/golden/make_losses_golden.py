#!/usr/bin/env python3
"""Generate tests/golden/losses_reference.json and losses_reference.npz (the
float64 logits and sampled feature values, as arrays) from the reference's own
src/training/losses.py.

Run on the CPU, where the read-only reference tree is (it does not exist on the
GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_losses_golden.py

``torch.manual_seed(WEIGHT_SEED); CombinedTTSLoss().eval()`` of the reference
is evaluated on every case of losses_cases.py twice: as written, in float32
("f32": what a user of the reference gets), and in float64 ("f64": a copy of
the module converted with .double(), float64 inputs, and float64 as torch's
default dtype around the call, because the reference builds its windows and
filter rows with default-dtype factories) - what the GPU result is compared
with.  |f32 - f64| / |f64| is the recorded spread, from which the tests take
their tolerances.

The spectral term is recorded as the reference gives it, but its spread is
taken from our own evaluation of the same formula (losses_cases.stft_loss) on
torch.stft spectra whose frame-0 imaginary parts are forced to +0 in both
precisions: with reflect padding frame 0 is symmetric about its centre, its
imaginary parts are rounding residue, and where re < 0 the angle is +pi or -pi
by that residue's sign, which would otherwise fill the spread with flips of
2 pi (the test accounts for those flips bin by bin instead).  The last frame
is symmetric in the same way when the length is 1 modulo the hop (the
1025-sample case) and is forced with frame 0 there, which only narrows the
bar (losses_cases.symmetric_frames).

Only data is written: key lists, scalars, the float64 logits, per feature map
its float64 mean |.|, max |.| and SAMPLES values at seeded indices, a
fingerprint of every weight tensor, and EarlyStopping's answers to a scripted
sequence.
"""
import copy
import importlib.util
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
REF_LOSSES = Path("/root/reference/src/training/losses.py")
sys.path.insert(0, str(HERE))

import losses_cases as lc  # noqa: E402


def load_reference():
    spec = importlib.util.spec_from_file_location("reference_losses", REF_LOSSES)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class default_dtype:
    def __init__(self, dt):
        self.dt = dt

    def __enter__(self):
        self.old = torch.get_default_dtype()
        torch.set_default_dtype(self.dt)

    def __exit__(self, *exc):
        torch.set_default_dtype(self.old)


def tens(x, dt):
    if x is None:
        return None
    t = torch.from_numpy(np.asarray(x))
    return t.to(dt) if t.is_floating_point() else t


def spread(f32, f64):
    return {k: (abs(f32[k] - v) / abs(v) if v != 0 else abs(f32[k])) for k, v in f64.items()}


def two_ways(models, fn):
    """fn(model, dtype) -> dict of floats, in float32 and in float64."""
    out = {}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        with default_dtype(dt), torch.no_grad():
            out[name] = {k: float(v) for k, v in fn(models[name], dt).items()}
    out["spread"] = spread(out["f32"], out["f64"])
    return out


def forced_spectral(pred, target, dt):
    """SpectralLoss's formula on torch.stft spectra with the symmetric frames' imaginary parts set to +0."""
    total = 0.0
    for n_fft in lc.N_FFTS:
        S = []
        for x in (pred, target):
            s = torch.stft(tens(x, dt).squeeze(1), n_fft=n_fft, hop_length=n_fft // 4,
                           window=torch.hann_window(n_fft, dtype=dt), return_complex=True)
            for t in lc.symmetric_frames(x.shape[-1], n_fft // 4):
                s[..., t] = torch.complex(s[..., t].real, torch.zeros_like(s[..., t].real))
            S.append(s)
        mag = (S[0].abs() - S[1].abs()).abs().mean()
        phase = (torch.angle(S[0]) - torch.angle(S[1])).abs().mean() * 0.1
        total = total + (mag + phase)
    return float(total / len(lc.N_FFTS))


def main():
    ref = load_reference()
    torch.manual_seed(lc.WEIGHT_SEED)
    m32 = ref.CombinedTTSLoss().eval()
    models = {"f32": m32, "f64": copy.deepcopy(m32).double()}
    arrays = {}  # float64: "<case>.logits<scale>", "<case>.s<scale>l<layer>" (the sampled feature values)
    doc = {"torch": torch.__version__, "numpy": np.__version__, "weight_seed": lc.WEIGHT_SEED, "cases": {}}

    sd = m32.state_dict()
    doc["state_dict"] = []
    for k, v in sd.items():
        total, total_sq = lc.fingerprint(v.numpy())
        doc["state_dict"].append({"key": k, "shape": list(v.shape), "sum": total, "sum_sq": total_sq})

    es = lc.EARLY_STOPPING
    stopper = ref.EarlyStopping(patience=es["patience"], min_delta=es["min_delta"])
    trace = []
    for x in es["sequence"]:
        stop = stopper(x)
        trace.append({"stop": bool(stop), "best_loss": stopper.best_loss, "wait": stopper.wait})
    d = ref.EarlyStopping()
    doc["early_stopping"] = {"trace": trace, "defaults": {"patience": d.patience, "min_delta": d.min_delta,
                                                          "best_loss": d.best_loss, "wait": d.wait}}

    for name in lc.DISC_CASES:
        pred, target = lc.audio_case(name)
        case = {}
        with default_dtype(torch.float64), torch.no_grad():
            outs, feats = models["f64"].adversarial_loss.discriminator(tens(target, torch.float64))
        for s, o in enumerate(outs):
            arrays[f"{name}.logits{s}"] = o.reshape(-1).numpy()
        case["logit_shapes"] = [list(o.shape) for o in outs]
        case["features"] = []
        for s, maps in enumerate(feats):
            row = []
            for l, f in enumerate(maps):
                flat = f.reshape(-1)
                idx = lc.sample_indices(s, l, flat.numel())
                arrays[f"{name}.s{s}l{l}"] = flat[torch.from_numpy(idx)].numpy()
                row.append({"shape": list(f.shape), "mean_abs": float(flat.abs().mean()),
                            "max_abs": float(flat.abs().max())})
            case["features"].append(row)
        case["feature_matching_normaliser"] = len(feats) * len(feats[0])

        def adversarial(model, dt):
            adv = model.adversarial_loss
            p, t = tens(pred, dt), tens(target, dt)
            return {"generator_loss": adv.generator_loss(p), "feature_matching_loss": adv.feature_matching_loss(t, p),
                    "discriminator_loss": adv.discriminator_loss(t, p)}
        case["adversarial"] = two_ways(models, adversarial)
        doc["cases"][name] = case

    keys = {}
    for name in lc.FULL_CASES:
        kw = lc.loss_case(name)
        case = doc["cases"][name]
        for mode, flag in (("generator", False), ("discriminator", True)):
            def run(model, dt, flag=flag):
                return model(**{k: tens(v, dt) for k, v in kw.items()}, optimize_discriminator=flag)
            case[mode] = two_ways(models, run)
            keys[mode] = list(case[mode]["f32"])
        f32, f64 = (forced_spectral(kw["audio_pred"], kw["audio_target"], dt) for dt in (torch.float32, torch.float64))
        case["spectral_forced"] = {"f32": f32, "f64": f64, "spread": abs(f32 - f64) / abs(f64)}

        def no_audio(model, dt):
            return model(**{k: tens(v, dt) for k, v in kw.items() if not k.startswith("audio")})
        case["no_audio"] = two_ways(models, no_audio)
        keys["no_audio"] = list(case["no_audio"]["f32"])
    doc["dict_keys"] = keys
    doc["training_step"] = m32.training_step

    (HERE / "losses_reference.json").write_text(json.dumps(doc) + "\n")
    np.savez_compressed(HERE / "losses_reference.npz", **arrays)
    worst = {}
    for name in lc.FULL_CASES:
        c = doc["cases"][name]
        for mode in ("generator", "discriminator", "no_audio"):
            for k, v in c[mode]["spread"].items():
                worst[k] = max(worst.get(k, 0.0), v)
        worst["spectral_forced"] = max(worst.get("spectral_forced", 0.0), c["spectral_forced"]["spread"])
    for name in lc.DISC_CASES:
        for k, v in doc["cases"][name]["adversarial"]["spread"].items():
            worst["adversarial " + k] = max(worst.get("adversarial " + k, 0.0), v)
    for k, v in sorted(worst.items()):
        print(f"{k:40s} {v:.3e}")


if __name__ == "__main__":
    main()
