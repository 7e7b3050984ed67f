"""Step time of ESRGANTrainStep with and without the Gram-matrix style term of the perceptual loss, in one process on one GPU.

configs[2] as bench.py runs it (B = 32, 8 Sentinel-2 frames = 24 input channels, fp32h, deterministic reductions, hipGraph replay) with
the shipped perceptual block (esrgan_s2naip_urban.yml:123-137, random VGG19 weights), once with style_weight 0 and once with
style_weight > 0.  The two steps are timed in alternating blocks (per-step event pairs), and the median of each is printed as one JSON
line.

  python tools/style_loss_bench.py [--steps 24] [--warmup 3] [--style-weight 1]
  python tools/style_loss_bench.py --only-style --steps 5          # under rocprofv3 --kernel-trace --stats
  python tools/style_loss_bench.py --analyze <kernel_trace.csv>    # per-tap Gram kernel times and their fraction of the MFMA ceiling
"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYER_WEIGHTS = {"conv1_2": 0.1, "conv2_2": 0.1, "conv3_4": 1, "conv4_4": 1, "conv5_4": 1}
TAPS = [("conv1_2", 64, 128 * 128), ("conv2_2", 128, 64 * 64), ("conv3_4", 256, 32 * 32), ("conv4_4", 512, 16 * 16), ("conv5_4", 512, 8 * 8)]
CEIL_TF = {"float": 155.0, "bf16": 2500.0}      # dense fp32 MFMA, bf16 MFMA (TFLOP/s)


def build(style_weight, B, dtype):
    from satlas_super_resolution_amd import flops, perceptual as P
    from satlas_super_resolution_amd.train_step import ESRGANTrainStep, StepConfig
    g_kw = dict(num_in_ch=24, num_out_ch=3, scale=4, num_feat=64, num_block=23, num_grow_ch=32)
    d_kw = dict(num_in_ch=3, num_feat=64, skip_connection=True)
    percep = {"type": "PerceptualLoss", "layer_weights": LAYER_WEIGHTS, "vgg_type": "vgg19", "use_input_norm": True, "perceptual_weight": 1.0,
              "style_weight": style_weight, "range_norm": False, "criterion": "l1"}
    ts = ESRGANTrainStep(g_kw, d_kw, B, 32, 32, dtype, StepConfig(perceptual=percep, deterministic=True), use_graph=True,
                         vgg_state=P.vgg19_random_state(P.vgg19_specs("conv5_4"), seed=2))
    ts.load_state(flops.generator_random_state(seed=0, **g_kw), flops.discriminator_random_state(3, 64, seed=1))
    return ts


def run(args):
    import torch
    torch.manual_seed(0)
    B = args.batch
    lr = torch.rand(B, 24, 32, 32, device="cuda")
    gt = torch.rand(B, 3, 128, 128, device="cuda")
    weights = [args.style_weight] if args.only_style else [0.0, args.style_weight]
    steps = {}
    for sw in weights:
        ts = build(sw, B, args.dtype)
        ts.feed_data(lr, gt)
        for _ in range(max(2, args.warmup)):
            ts.step()
        steps[sw] = ts
    torch.cuda.synchronize()
    times = {sw: [] for sw in weights}
    block = 4
    while min(len(v) for v in times.values()) < args.steps:
        for sw, ts in steps.items():
            for _ in range(block):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                ts.step()
                b.record()
                b.synchronize()
                times[sw].append(a.elapsed_time(b))
    logs = {sw: ts.log() for sw, ts in steps.items()}
    out = {"what": "ESRGANTrainStep configs[2] + perceptual block, style term off / on", "batch": B, "dtype": args.dtype,
           "deterministic": True, "hip_graph": True, "timed_steps_each": {str(k): len(v) for k, v in times.items()},
           "median_ms": {f"style_weight={k:g}": round(statistics.median(v), 4) for k, v in times.items()},
           "min_ms": {f"style_weight={k:g}": round(min(v), 4) for k, v in times.items()},
           "l_g_style": {f"style_weight={k:g}": v.get("l_g_style") for k, v in logs.items()}}
    if not args.only_style:
        out["style_term_ms"] = round(statistics.median(times[args.style_weight]) - statistics.median(times[0.0]), 4)
    print(json.dumps(out))


def analyze(path, B):
    """per-tap mean duration of the Gram kernels in a rocprofv3 kernel trace; dispatches come in tap order within each launch group"""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            if "gram_" in name:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), name))
    rows.sort()
    groups = {}
    for _, dur, name in rows:
        kind = "fwd" if "gram_fwd_kernel" in name else "reduce" if "gram_reduce" in name else "l1" if "gram_l1" in name else "bwd"
        tdt = "bf16" if ("__bf16" in name or "DF16b" in name) else "float"
        groups.setdefault((kind, tdt), []).append(dur)
    res = []
    for (kind, tdt), durs in sorted(groups.items()):
        if kind in ("fwd", "bwd"):
            # fwd: 5 target + 5 output Grams per step; bwd: 5 per step; both in tap order
            for ti, (tap, C, P) in enumerate(TAPS):
                mine = durs[ti::5]
                us = statistics.mean(mine) / 1e3
                fl = (C * C * P * B) if kind == "fwd" else (2 * C * C * P * B)   # fwd: the symmetric half of 2 C^2 P per image
                tf = fl / (us * 1e-6) / 1e12
                res.append({"kernel": f"gram_{kind}<{tdt}>", "tap": tap, "C": C, "HW": P, "calls": len(mine), "mean_us": round(us, 2),
                            "gflop": round(fl / 1e9, 3), "tflops": round(tf, 1), "fraction_of_ceiling": round(tf / CEIL_TF[tdt], 3)})
        else:
            res.append({"kernel": f"gram_{kind}<{tdt}>", "calls": len(durs), "mean_us": round(statistics.mean(durs) / 1e3, 2)})
    for r in res:
        print(json.dumps(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="fp32h")
    ap.add_argument("--style-weight", type=float, default=1.0)
    ap.add_argument("--only-style", action="store_true")
    ap.add_argument("--analyze", metavar="KERNEL_TRACE_CSV")
    args = ap.parse_args()
    if args.analyze:
        analyze(args.analyze, args.batch)
    else:
        os.environ.setdefault("SSR_VGG19_RANDOM", "1")
        run(args)


if __name__ == "__main__":
    main()
