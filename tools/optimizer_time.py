"""Step time of ESRGANTrainStep with the default optimizer (plain Adam on both networks: ssr_adam_step_guarded) and with AdamW + amsgrad on
both networks (ssr_optim_step_guarded, csrc/optim.hip: three state arenas, the heaviest kind in memory traffic), in one process on one GPU.

configs[2] as bench.py runs it (B = 32, 8 Sentinel-2 frames = 24 input channels, fp32h, deterministic reductions, hipGraph replay, no
perceptual block).  The legs are timed in alternating blocks (per-step event pairs), as tools/loss_variants_time.py does; medians, minima
and the default leg's own block medians are printed as one JSON line.  `--default-only` puts a second instance of the default step in the
other leg's place, so that the default leg's blocks alternate with another model's blocks all the same: the form that also runs on a
tree from before the feature.  There is no CPU path.

  python tools/optimizer_time.py [--steps 24] [--warmup 3] [--default-only]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ADAMW = dict(type="AdamW", lr=1e-4, betas=(0.9, 0.99), weight_decay=0.01, amsgrad=True)


def build(variant, B, dtype):
    from satlas_super_resolution_amd import flops
    from satlas_super_resolution_amd.train_step import ESRGANTrainStep, StepConfig
    g_kw = dict(num_in_ch=24, num_out_ch=3, scale=4, num_feat=64, num_block=23, num_grow_ch=32)
    d_kw = dict(num_in_ch=3, num_feat=64, skip_connection=True)
    cfg = StepConfig(deterministic=True)
    if variant:
        from satlas_super_resolution_amd import optimizers
        cfg.optim_g, cfg.optim_d = optimizers.normalize_optim("optim_g", ADAMW), optimizers.normalize_optim("optim_d", ADAMW)
    ts = ESRGANTrainStep(g_kw, d_kw, B, 32, 32, dtype, cfg, use_graph=True)
    ts.load_state(flops.generator_random_state(seed=0, **g_kw), flops.discriminator_random_state(3, 64, seed=1))
    return ts


def run(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/optimizer_time.py needs a GPU: the train step has no CPU path")
    torch.manual_seed(0)
    B = args.batch
    lr = torch.rand(B, 24, 32, 32, device="cuda")
    gt = torch.rand(B, 3, 128, 128, device="cuda")
    legs = {"Adam (default)": False}
    legs["Adam (second instance)" if args.default_only else "AdamW + amsgrad"] = not args.default_only
    steps = {}
    for name, variant in legs.items():
        ts = build(variant, B, args.dtype)
        ts.feed_data(lr, gt)
        for _ in range(max(2, args.warmup)):
            ts.step()
        steps[name] = ts
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    block = 4
    while min(len(v) for v in times.values()) < args.steps:
        for name, ts in steps.items():
            for _ in range(block):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                ts.step()
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b))
    default = list(legs)[0]
    blocks = [statistics.median(times[default][i:i + block]) for i in range(0, len(times[default]), block)]
    out = {"what": "ESRGANTrainStep configs[2], optimizer legs", "batch": B, "dtype": args.dtype, "deterministic": True, "hip_graph": True,
           "timed_steps_each": {k: len(v) for k, v in times.items()},
           "median_ms": {k: round(statistics.median(v), 4) for k, v in times.items()},
           "min_ms": {k: round(min(v), 4) for k, v in times.items()},
           "default_block_medians_ms": [round(x, 4) for x in blocks],
           "optimizer_state_arenas": {k: list(getattr(ts.opt_g, "arenas", {"exp_avg": 0, "exp_avg_sq": 0})) for k, ts in steps.items()},
           "log": {k: {n: round(v, 6) for n, v in ts.log().items()} for k, ts in steps.items()}}
    variant = list(legs)[1]
    if not args.default_only:
        out["variant_minus_default_ms"] = round(statistics.median(times[variant]) - statistics.median(times[default]), 4)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24, help="timed steps of each leg (at least)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="fp32h")
    ap.add_argument("--default-only", action="store_true")
    run(ap.parse_args())


if __name__ == "__main__":
    main()
