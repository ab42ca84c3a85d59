#!/usr/bin/env python3
"""What a ragged batch costs: M2TTSModel.inference_ragged against the padded
batch and against the single-utterance calls, alternated within one process.

Workloads (the bench configurations' B and S): explicit integer durations give
utterance b its own frame count T_b, spread evenly over [T_max / 2, T_max].
    (a) ragged   inference_ragged(ids, lens, durations=d)
    (b) padded   forward(ids, lens, target_durations=d): every utterance
                 decoded and vocoded over T_max rows (the reference's batch)
    (c) singles  B forward calls of one utterance each
After a settling phase that runs all three, each round times `--iters` calls of
each variant in turn (host clock around a device synchronise); the figure of a
variant is the median of its rounds, with the spread beside it.

    python3 tools/probe/ragged_timing.py --stage s2 --batch 8 [--out FILE.json]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- \\
        python3 tools/probe/ragged_timing.py --stage s2 --batch 8 --only ragged --rounds 1
(the second form, a run of its own, gives ragged_tail_kernel's time beside the
vocoder's kernels in DIR's kernel statistics).
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "m2-tts_amd" / "src"))
sys.path.insert(0, str(ROOT))


def spread_durations(B: int, S: int, t_max: int) -> torch.Tensor:
    """[B, S] integer durations whose row sums go evenly from t_max / 2 to t_max."""
    d = torch.zeros(B, S)
    for b in range(B):
        t = t_max if B == 1 else round(t_max / 2 + (t_max - t_max / 2) * b / (B - 1))
        d[b] = t // S
        d[b, :t % S] += 1
    return d


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--stage", choices=["s1", "s2"], default="s2")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=100)
    ap.add_argument("--tmax", type=int, default=500)
    ap.add_argument("--iters", type=int, default=20, help="calls per variant per round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--settle-ms", type=float, default=1500.0)
    ap.add_argument("--only", choices=["ragged", "padded", "singles"], default=None)
    ap.add_argument("--out", type=str, default=None, help="write the result as JSON here")
    args = ap.parse_args(argv)

    import bench
    if not torch.cuda.is_available():
        raise SystemExit("ragged_timing: needs a ROCm GPU (no CPU path)")
    dev = torch.device("cuda", 0)
    m = bench.fixture_model(bench.STAGE1 if args.stage == "s1" else bench.STAGE2, dev)
    B, S = args.batch, args.seq
    ids = torch.randint(1, 40, (B, S), generator=torch.Generator().manual_seed(5)).to(dev)
    lens = torch.full((B,), S, dtype=torch.int64, device=dev)
    d = spread_durations(B, S, args.tmax).to(dev)
    frames = [int(x) for x in d.sum(1).tolist()]
    rows = [(ids[b:b + 1], lens[b:b + 1], d[b:b + 1]) for b in range(B)]

    def ragged():
        return m.inference_ragged(ids, lens, durations=d)

    def padded():
        return m(ids, lens, target_durations=d)

    def singles():
        return [m(i, n, target_durations=x) for i, n, x in rows]

    variants = {"ragged": ragged, "padded": padded, "singles": singles}
    if args.only:
        variants = {args.only: variants[args.only]}
    with torch.no_grad():
        _, _, got = m.inference_ragged(ids, lens, durations=d)
        assert got.tolist() == frames, (got.tolist(), frames)
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.settle_ms:  # warm every shape, settle the clocks
            for fn in variants.values():
                fn()
            torch.cuda.synchronize(dev)
        ms = {k: [] for k in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    fn()
                torch.cuda.synchronize(dev)
                ms[name].append((time.perf_counter() - t0) * 1e3 / args.iters)
    res = {"stage": args.stage, "B": B, "S": S, "T_max": args.tmax, "frames": frames, "iters": args.iters,
           "rounds": args.rounds, "device": torch.cuda.get_device_name(dev),
           "ms_per_call": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()}}
    for k, v in res["ms_per_call"].items():
        print(f"{args.stage} B={B} S={S} T_max={args.tmax} {k:8s} {v['median']:.4f} ms per call "
              f"(rounds {v['min']:.4f} .. {v['max']:.4f})")
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
