#!/usr/bin/env python3
"""In-process A/B of several builds of the library on one vocoder call shape
(build defines, or a parent commit's build: what voc_env_ab.py does for an
M2_* switch).  Every build is loaded into ONE process with a model handle of
its own; the builds alternate every `steps` calls for `rounds` rounds, each
block timed with events on the launch stream, and every build's audio is
checked bit-equal to the first one's.
    python tools/probe/voc_lib_ab.py name=lib.so,name=lib.so,... path(1=exact-f32|2=split) stage B T [rounds] [steps]"""
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "m2-tts_amd" / "src"))
sys.path.insert(0, str(ROOT))


def main():
    import bench
    from m2amd import _lib
    builds = [b.split("=", 1) for b in sys.argv[1].split(",")]
    path, stage = int(sys.argv[2]), sys.argv[3]
    B, T = int(sys.argv[4]), int(sys.argv[5])
    rounds = int(sys.argv[6]) if len(sys.argv) > 6 else 8
    steps = int(sys.argv[7]) if len(sys.argv) > 7 else 200
    dev = torch.device("cuda", 0)
    cfg = bench.STAGE1 if stage == "s1" else bench.STAGE2
    mel = torch.randn(B, cfg["mel_channels"], T, generator=torch.Generator().manual_seed(11)).to(dev)
    libs, models = {}, {}

    def use(name):  # every call of m2amd goes through _lib.load(), which returns _lib._lib
        _lib._lib = libs[name]

    for name, p in builds:
        _lib._lib = None
        libs[name] = _lib.load(Path(p))
        models[name] = bench.fixture_model(cfg, dev)
        models[name]._hip(dev).vocoder_select(path)
    ref = None
    for name, _ in builds:
        use(name)
        a = models[name].vocoder(mel)
        torch.cuda.synchronize()
        if ref is None:
            ref = a.clone()
        print(f"{name}: bit-equal to {builds[0][0]}: {torch.equal(a, ref)}  max-abs {(a - ref).abs().max().item():.3g}",
              flush=True)
    use(builds[0][0])
    t_end = time.perf_counter() + 0.6  # clock settling (bench.py settle_ms)
    while time.perf_counter() < t_end:
        models[builds[0][0]].vocoder(mel)
        torch.cuda.synchronize()
    res = {name: [] for name, _ in builds}
    for _ in range(rounds):
        for name, _p in builds:
            use(name)
            m = models[name]
            m.vocoder(mel)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                m.vocoder(mel)
            e1.record()
            e1.synchronize()
            res[name].append(e0.elapsed_time(e1) / steps)
    for name, _ in builds:
        x = sorted(res[name])
        print(f"{name} path {path} {stage} B={B} T={T}: median {x[len(x) // 2]:.5f} ms/call  min {x[0]:.5f}  "
              f"all {[round(t, 5) for t in res[name]]}", flush=True)
    first = res[builds[0][0]]
    for name, _ in builds[1:]:
        wins = sum(a < b for a, b in zip(res[name], first))
        print(f"{name} faster than {builds[0][0]} in {wins} of {rounds} pairs", flush=True)
    import gc
    torch.cuda.synchronize()
    m = None
    for name, _ in builds:  # every handle is destroyed by the build that made it
        use(name)
        del models[name]
        gc.collect()


if __name__ == "__main__":
    main()
