"""Step time of ESRGANTrainStep with and without the SSIM term (train.ssim_opt, csrc/ssim.hip), in one process on one GPU.

configs[2] as bench.py runs it (B = 32, 8 Sentinel-2 frames = 24 input channels, fp32h, deterministic reductions, hipGraph replay) with
the shipped perceptual block (esrgan_s2naip_urban.yml:123-137, random VGG19 weights), once without `ssim` and once with the shipped
ssimloss block's weight (ssimloss_esrgan_s2naip_urban.yml: 0.1).  The two steps are timed in alternating blocks (per-step event pairs),
and medians and minima are printed as one JSON line.  There is no CPU path: without a GPU the script fails.

  python tools/ssim_loss_bench.py [--steps 24] [--warmup 3] [--ssim-weight 0.1]
  python tools/ssim_loss_bench.py --only-ssim --steps 5          # under rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYER_WEIGHTS = {"conv1_2": 0.1, "conv2_2": 0.1, "conv3_4": 1, "conv4_4": 1, "conv5_4": 1}


def build(ssim_weight, B, dtype):
    from satlas_super_resolution_amd import flops, perceptual as P
    from satlas_super_resolution_amd.train_step import ESRGANTrainStep, StepConfig
    g_kw = dict(num_in_ch=24, num_out_ch=3, scale=4, num_feat=64, num_block=23, num_grow_ch=32)
    d_kw = dict(num_in_ch=3, num_feat=64, skip_connection=True)
    percep = {"type": "PerceptualLoss", "layer_weights": LAYER_WEIGHTS, "vgg_type": "vgg19", "use_input_norm": True, "perceptual_weight": 1.0,
              "style_weight": 0, "range_norm": False, "criterion": "l1"}
    cfg = StepConfig(perceptual=percep, deterministic=True, ssim={"loss_weight": ssim_weight} if ssim_weight else None)
    ts = ESRGANTrainStep(g_kw, d_kw, B, 32, 32, dtype, cfg, use_graph=True, vgg_state=P.vgg19_random_state(P.vgg19_specs("conv5_4"), seed=2))
    ts.load_state(flops.generator_random_state(seed=0, **g_kw), flops.discriminator_random_state(3, 64, seed=1))
    return ts


def run(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/ssim_loss_bench.py needs a GPU: the train step has no CPU path")
    torch.manual_seed(0)
    B = args.batch
    lr = torch.rand(B, 24, 32, 32, device="cuda")
    gt = torch.rand(B, 3, 128, 128, device="cuda")
    weights = [args.ssim_weight] if args.only_ssim else [0.0, args.ssim_weight]
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
    name = lambda k: "ssim off" if not k else f"ssim loss_weight={k:g}"     # noqa: E731
    out = {"what": "ESRGANTrainStep configs[2] + perceptual block, SSIM term off / on", "batch": B, "dtype": args.dtype,
           "deterministic": True, "hip_graph": True, "timed_steps_each": {name(k): len(v) for k, v in times.items()},
           "median_ms": {name(k): round(statistics.median(v), 4) for k, v in times.items()},
           "min_ms": {name(k): round(min(v), 4) for k, v in times.items()},
           "l_g_ssim": {name(k): v.get("l_g_ssim") for k, v in logs.items()}}
    if not args.only_ssim:
        out["ssim_term_ms"] = round(statistics.median(times[args.ssim_weight]) - statistics.median(times[0.0]), 4)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24, help="timed steps of each leg (at least)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="fp32h")
    ap.add_argument("--ssim-weight", type=float, default=0.1)
    ap.add_argument("--only-ssim", action="store_true")
    args = ap.parse_args()
    if args.ssim_weight <= 0:
        ap.error("--ssim-weight must be positive")
    os.environ.setdefault("SSR_VGG19_RANDOM", "1")
    run(args)


if __name__ == "__main__":
    main()
