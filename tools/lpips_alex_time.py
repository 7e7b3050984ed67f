"""Time per 128 x 128 image pair of the LPIPS metric with the AlexNet backbone beside the VGG backbone (lpips_metric.lpips_distance,
random weights of each architecture), in ONE process: alternating blocks of calls, per backbone the median over all its calls and
the spread of its blocks' medians.  Device times are HIP-event pairs around whole calls (the download of the partials included),
after a warm-up of both.  One JSON line.  There is no CPU path.

  python tools/lpips_alex_time.py [--blocks 6] [--reps 20] [--warmup 5]
  python tools/lpips_alex_time.py --trace     # under rocprofv3 --kernel-trace --stats (a run of its own): few AlexNet calls only
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def block(fn, reps):
    import torch
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def run(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/lpips_alex_time.py needs a GPU: the metric has no CPU path")
    from satlas_super_resolution_amd import lpips_metric as LM
    g = torch.Generator().manual_seed(0)
    a = torch.randint(0, 256, (1, 128, 128, 3), generator=g, dtype=torch.uint8)
    b = (a.int() + torch.randint(-8, 9, a.shape, generator=g, dtype=torch.int32)).clamp(0, 255).to(torch.uint8)
    ad, bd = a.cuda(), b.cuda()
    nets = ("alex",) if args.trace else ("alex", "vgg")
    models = {n: LM.LPIPSModel(LM.lpips_random_state(0, net=n), "cuda", net=n) for n in nets}
    calls = {n: (lambda m=models[n]: LM.lpips_distance(ad, bd, m)) for n in nets}
    for n in nets:
        block(calls[n], 2 if args.trace else args.warmup)
    torch.cuda.synchronize()
    if args.trace:
        block(calls["alex"], 4)
        print(json.dumps({"what": "lpips_distance, AlexNet backbone, 1 x 128 x 128: 6 calls for a kernel trace"}))
        return
    ts = {n: [] for n in nets}
    for _ in range(args.blocks):
        for n in nets:
            ts[n].append(block(calls[n], args.reps))
    out = {"what": "lpips_distance per 128 x 128 pair, alternating blocks in one process", "blocks": args.blocks, "reps_per_block": args.reps}
    for n in nets:
        meds = [statistics.median(t) for t in ts[n]]
        out[n] = {"median_ms": round(statistics.median([v for t in ts[n] for v in t]), 4),
                  "block_medians_min_ms": round(min(meds), 4), "block_medians_max_ms": round(max(meds), 4)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", action="store_true", help="few calls of the AlexNet backbone only (for a kernel trace)")
    run(ap.parse_args())


if __name__ == "__main__":
    main()
