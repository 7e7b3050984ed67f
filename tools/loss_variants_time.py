"""Step time of ESRGANTrainStep with the default losses (L1Loss + vanilla: ssr_l1_loss, ssr_bce_logits_loss) and with hinge + MSELoss
(ssr_gan_loss, ssr_pixel_loss: csrc/losses.hip), in one process on one GPU.

configs[2] as bench.py runs it (B = 32, 8 Sentinel-2 frames = 24 input channels, fp32h, deterministic reductions, hipGraph replay, no
perceptual block).  The two steps are timed in alternating blocks (per-step event pairs), as tools/ssim_loss_bench.py does, and
medians and minima are printed as one JSON line, with the spread of the default leg's own blocks beside the difference.  There is no
CPU path: without a GPU the script fails.

  python tools/loss_variants_time.py [--steps 24] [--warmup 3] [--gan-type hinge] [--pixel-type MSELoss]
  python tools/loss_variants_time.py --steps 4          # under rocprofv3 --kernel-trace --stats: the four loss kernels' own times
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(gan_type, pixel_type, B, dtype):
    from satlas_super_resolution_amd import flops
    from satlas_super_resolution_amd.train_step import ESRGANTrainStep, StepConfig
    g_kw = dict(num_in_ch=24, num_out_ch=3, scale=4, num_feat=64, num_block=23, num_grow_ch=32)
    d_kw = dict(num_in_ch=3, num_feat=64, skip_connection=True)
    cfg = StepConfig(deterministic=True, gan_type=gan_type, pixel_type=pixel_type)
    ts = ESRGANTrainStep(g_kw, d_kw, B, 32, 32, dtype, cfg, use_graph=True)
    ts.load_state(flops.generator_random_state(seed=0, **g_kw), flops.discriminator_random_state(3, 64, seed=1))
    return ts


def run(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/loss_variants_time.py needs a GPU: the train step has no CPU path")
    torch.manual_seed(0)
    B = args.batch
    lr = torch.rand(B, 24, 32, 32, device="cuda")
    gt = torch.rand(B, 3, 128, 128, device="cuda")
    legs = {"L1Loss + vanilla": ("vanilla", "L1Loss"), f"{args.pixel_type} + {args.gan_type}": (args.gan_type, args.pixel_type)}
    steps = {}
    for name, (gan_type, pixel_type) in legs.items():
        ts = build(gan_type, pixel_type, B, args.dtype)
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
    default, variant = list(legs)
    blocks = [statistics.median(times[default][i:i + block]) for i in range(0, len(times[default]), block)]
    out = {"what": "ESRGANTrainStep configs[2], default losses / loss variants", "batch": B, "dtype": args.dtype, "deterministic": True,
           "hip_graph": True, "timed_steps_each": {k: len(v) for k, v in times.items()},
           "median_ms": {k: round(statistics.median(v), 4) for k, v in times.items()},
           "min_ms": {k: round(min(v), 4) for k, v in times.items()},
           "variant_minus_default_ms": round(statistics.median(times[variant]) - statistics.median(times[default]), 4),
           "default_block_medians_spread_ms": round(max(blocks) - min(blocks), 4),
           "log": {k: {n: round(v, 6) for n, v in ts.log().items()} for k, ts in steps.items()}}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24, help="timed steps of each leg (at least)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="fp32h")
    ap.add_argument("--gan-type", default="hinge", choices=["lsgan", "wgan", "wgan_softplus", "hinge"])
    ap.add_argument("--pixel-type", default="MSELoss", choices=["MSELoss", "CharbonnierLoss"])
    run(ap.parse_args())


if __name__ == "__main__":
    main()
