"""Step time of ESRGANTrainStep without the CLIP loss and with it under both tower arithmetics and both tower attentions
(train.clip_opt; clip_loss.py, csrc/vit_bwd.hip, csrc/linear_split.hip, csrc/mha_mfma.hip), in one process on one GPU.

The default step as bench.py runs it (B = 32, 8 Sentinel-2 frames = 24 input channels, fp32h, deterministic reductions, hipGraph
replay), once without `clip` and once per tower arithmetic with a random tower of the ViT-B-16-SigLIP-256 sizes (clip_random_state:
width 768, depth 12, 12 heads of 64, MLP 3072, patch 16, 256 tokens at 256 x 256).  The legs - off, exact, split and, with
`--tower-attention fma mfma`, exact+mfma and split+mfma - are timed in alternating blocks of three steps (per-step event pairs);
medians, minima and, per leg, the spread of its own blocks' medians are printed as one JSON line.  There is no CPU path: without a
GPU the script fails.

  python tools/clip_loss_bench.py [--steps 12] [--warmup 3] [--tower-arithmetic exact|split|both] [--tower-attention fma mfma]
  python tools/clip_loss_bench.py --only-clip --tower-arithmetic split --steps 3 --no-graph   # under rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOWER = dict(width=768, depth=12, mlp=3072, patch=16, grid=16, heads=12)
BLOCK = 3


def build(leg, B, dtype, use_graph):
    """leg: 'off' | 'exact' | 'split' | 'exact+mfma' | 'split+mfma'"""
    from satlas_super_resolution_amd import clipscore_metric as CM, flops
    from satlas_super_resolution_amd.train_step import ESRGANTrainStep, StepConfig
    g_kw = dict(num_in_ch=24, num_out_ch=3, scale=4, num_feat=64, num_block=23, num_grow_ch=32)
    d_kw = dict(num_in_ch=3, num_feat=64, skip_connection=True)
    clip = None
    if leg != "off":
        clip = {"model": "ViT-B-16-SigLIP-256", "family": "siglip", "path": None, "gelu": "tanh", "loss_weight": 1.0}
        if leg.startswith("split"):
            clip["tower_arithmetic"] = "split"
        if leg.endswith("+mfma"):
            clip["tower_attention"] = "mfma"
    cfg = StepConfig(deterministic=True, clip=clip)
    ts = ESRGANTrainStep(g_kw, d_kw, B, 32, 32, dtype, cfg, use_graph=use_graph,
                         clip_state=CM.clip_random_state("siglip", seed=3, **TOWER) if clip else None)
    ts.load_state(flops.generator_random_state(seed=0, **g_kw), flops.discriminator_random_state(3, 64, seed=1))
    return ts


def tower_flops(B):
    """multiply-adds x 2 of the linear launches of one step's term: two forwards (target, generated) and one data-gradient pass"""
    w, d, m, T, kp = TOWER["width"], TOWER["depth"], TOWER["mlp"], TOWER["grid"] ** 2, 3 * TOWER["patch"] ** 2
    per_token = kp * w + d * (4 * w * w + 2 * w * m) + 2 * w * w          # embedding, blocks (qkv 3, proj 1, fc1, fc2), pooling kv
    return 2.0 * 3 * B * T * per_token


def run(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/clip_loss_bench.py needs a GPU: the train step has no CPU path")
    torch.manual_seed(0)
    B = args.batch
    lr = torch.rand(B, 24, 32, 32, device="cuda")
    gt = torch.rand(B, 3, 128, 128, device="cuda")
    arith = ["exact", "split"] if args.tower_arithmetic == "both" else [args.tower_arithmetic]
    on = [a + ("+mfma" if t == "mfma" else "") for a in arith for t in args.tower_attention]      # each fma leg beside its mfma leg
    legs = on if args.only_clip else ["off"] + on
    steps = {}
    for leg in legs:
        ts = build(leg, B, args.dtype, not args.no_graph)
        ts.feed_data(lr, gt)
        for _ in range(max(2, args.warmup)):
            ts.step()
        steps[leg] = ts
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    while min(len(v) for v in times.values()) < args.steps:
        for k, ts in steps.items():
            for _ in range(BLOCK):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                ts.step()
                b.record()
                b.synchronize()
                times[k].append(a.elapsed_time(b))
    logs = {k: ts.log() for k, ts in steps.items()}
    name = lambda k: f"clip {k}"                                             # noqa: E731
    med = {k: statistics.median(v) for k, v in times.items()}
    blocks = {k: [statistics.median(v[i:i + BLOCK]) for i in range(0, len(v), BLOCK)] for k, v in times.items()}
    out = {"what": "ESRGANTrainStep, the default benchmark step, CLIP loss off / on with tower_arithmetic exact / split and "
                   "tower_attention fma (no suffix) / mfma (random ViT-B-16-SigLIP-256-sized tower)", "batch": B,
           "dtype": args.dtype, "deterministic": True, "hip_graph": not args.no_graph, "timed_steps_each": {name(k): len(v) for k, v in times.items()},
           "median_ms": {name(k): round(med[k], 3) for k in times},
           "min_ms": {name(k): round(min(v), 3) for k, v in times.items()},
           "block_medians_ms": {name(k): [round(x, 3) for x in v] for k, v in blocks.items()},
           "block_spread_ms": {name(k): round(max(v) - min(v), 3) for k, v in blocks.items()},
           "l_clip_sim": {name(k): logs[k].get("l_clip_sim") for k in on},
           "term_launches": {name(k): len(steps[k].c_plan.launcher) for k in on},
           "saved_activation_bytes": steps[on[0]].c_plan.saved_bytes,
           "term_linear_gflop": round(tower_flops(B) / 1e9, 1), "device_memory_allocated_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    if not args.only_clip:
        out["clip_term_ms"] = {name(k): round(med[k] - med["off"], 3) for k in on}
        out["term_linear_tflops"] = {name(k): round(tower_flops(B) / 1e9 / (med[k] - med["off"]), 1) for k in on}
        if "exact" in on and "split" in on:
            out["split_saves_ms"] = round(med["exact"] - med["split"], 3)
    spread = out["block_spread_ms"]
    for a in arith:                                                          # mfma against fma, beside the larger of the two legs' own spreads
        if a in on and a + "+mfma" in on:
            out.setdefault("mfma_saves_ms", {})[name(a)] = round(med[a] - med[a + "+mfma"], 3)
            out.setdefault("mfma_pair_spread_ms", {})[name(a)] = max(spread[name(a)], spread[name(a + "+mfma")])
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12, help="timed steps of each leg (at least)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="fp32h")
    ap.add_argument("--tower-arithmetic", default="both", choices=["exact", "split", "both"],
                    help="the arithmetic of the tower's matrix products in the legs with the term (both: one leg each)")
    ap.add_argument("--tower-attention", nargs="+", default=["fma"], choices=["fma", "mfma"],
                    help="the kernels of the blocks' self-attention in the legs with the term (fma mfma: one leg each per arithmetic)")
    ap.add_argument("--only-clip", action="store_true")
    ap.add_argument("--no-graph", action="store_true")
    run(ap.parse_args())


if __name__ == "__main__":
    main()
