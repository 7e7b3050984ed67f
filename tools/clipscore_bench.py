"""Time of one CLIPScore pair (two 128 x 128 images, one pass of batch 2) for both real-size towers with random weights
(clipscore_metric.clip_random_state), HIP events, one process.

    python tools/clipscore_bench.py [--towers siglip clip] [--tower-arithmetic exact split] [--tower-attention fma mfma] [--iters 10] [--warmup 3] [--out FILE.json]

Prints one JSON line per tower, tower arithmetic and tower attention (fma: ssr_mha_fwd | mfma: ssr_mha_mfma_fwd for the blocks): ms per pair (median, min, max), the FLOPs of the ssr_linear / ssr_linear_split
launches of the plan (2 M K Nout each) and what share of the matrix-core ceiling (155 TFLOP/s fp32 MFMA for `exact`; 833 TFLOP/s =
a third of the 16-bit rate for `split`, which spends three MFMAs per product) the WHOLE pair time would be if it were all linear
launches (a lower bound of the kernel's own fraction: the kernel trace under profiles/clipscore/ splits the time by kernel)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP32_MFMA_TFLOPS = 155.0
CEILING_TFLOPS = {"exact": FP32_MFMA_TFLOPS, "split": 2500.0 / 3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--towers", nargs="+", default=["siglip", "clip"])
    ap.add_argument("--tower-arithmetic", nargs="+", default=["exact"], choices=["exact", "split"])
    ap.add_argument("--tower-attention", nargs="+", default=["fma"], choices=["fma", "mfma"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from satlas_super_resolution_amd import clipscore_metric as CM, hip
    lib = hip.lib()
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (1, a.size, a.size, 3), generator=g, dtype=torch.uint8).cuda()
    img2 = torch.randint(0, 256, (1, a.size, a.size, 3), generator=g, dtype=torch.uint8).cuda()
    results = []
    for family, arith, attn in ((f, t, m) for f in a.towers for t in a.tower_arithmetic for m in a.tower_attention):
        state = CM.clip_random_state(family, seed=1)
        cfg = CM.vit_config_from_state(state)
        model = CM.CLIPVisualModel(state, "cuda", tower_arithmetic=arith, tower_attention=attn)
        del state
        plan = model.plan(2, a.size, a.size)
        calls = list(plan.launcher.flat_calls())
        lin = [args for fn, args, _ in calls if fn is lib.ssr_linear or fn is lib.ssr_linear_split]
        flops = sum(2 * args[6] * args[7] * args[8] for args in lin)
        for _ in range(a.warmup):
            s = CM.clipscore(img, img2, model)
        times = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            s = CM.clipscore(img, img2, model)            # includes the download of the score, as the metric entry does
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        times.sort()
        med = times[len(times) // 2]
        r = {"tower": family, "tower_arithmetic": arith, "tower_attention": attn, "width": cfg["width"], "depth": cfg["depth"], "tokens": cfg["tokens"], "image_size": cfg["image_size"],
             "pair_ms_median": round(med, 3), "pair_ms_min": round(times[0], 3), "pair_ms_max": round(times[-1], 3), "iters": a.iters,
             "launches": len(calls) + 1, "linear_launches": len(lin), "linear_gflop_per_pair": round(flops / 1e9, 2),
             "linear_tflops_if_all_time_were_linear": round(flops / (med * 1e-3) / 1e12, 2),
             "fraction_of_fp32_mfma_ceiling_lower_bound": round(flops / (med * 1e-3) / 1e12 / FP32_MFMA_TFLOPS, 4),
             "fraction_of_its_own_ceiling_lower_bound": round(flops / (med * 1e-3) / 1e12 / CEILING_TFLOPS[arith], 4),
             "score": float(s[0]), "device": hip.device_info()}
        print(json.dumps(r), flush=True)
        results.append(r)
        del model, plan
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
