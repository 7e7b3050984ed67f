"""Forward + backward time of OSMObjDiscriminator at the shape of osm_obj_esrgan.yml, beside SSR_UNetDiscriminatorSN at the same x.

    python tools/osm_disc_bench.py [--mode fp32h] [--warmup 3] [--blocks 6] [--steps 8]
    python tools/osm_disc_bench.py --profile-steps 3 [--only osm|unet]      # a short run for a kernel trace (no timing)

num_in_ch = 27, num_feat = 64, x [16, 27, 128, 128], osm_objs [16, 3, 32, 32] (batch 4 x n_osm_objs 4).  One process; the two networks
ALTERNATE in blocks (A B A B ...), every block `steps` training forwards + backwards with parameter and input gradients between two
device events.  The baseline is the existing network, never the new code against itself: what is reported is the difference of the two
medians beside the spread of the baseline's own blocks.  Not part of bench.py; one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="fp32h")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--objs", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--profile-steps", type=int, default=0)
    ap.add_argument("--only", default="both", choices=("both", "osm", "unet"))
    a = ap.parse_args()
    from satlas_super_resolution_amd import archs  # noqa: F401
    from satlas_super_resolution_amd.registry import ARCH_REGISTRY
    torch.manual_seed(0)
    osm = ARCH_REGISTRY.get("OSMObjDiscriminator")(27, num_feat=64, compute_dtype=a.mode)
    with torch.no_grad():              # gamma = 0 is the initial value; any other costs the same
        osm.o_attention1.gamma.fill_(0.7)
        osm.o_attention2.gamma.fill_(-0.4)
    unet = ARCH_REGISTRY.get("SSR_UNetDiscriminatorSN")(27, num_feat=64, compute_dtype=a.mode)
    osm, unet = osm.cuda().train(), unet.cuda().train()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(a.batch, 27, 128, 128, generator=g).cuda().requires_grad_(True)
    objs = torch.rand(a.objs, 3, 32, 32, generator=g).cuda().requires_grad_(True)

    def step_osm():
        out, o_out = osm(x, objs)
        (out.mean() + o_out.mean()).backward()

    def step_unet():
        unet(x).mean().backward()

    legs = [(n, f) for n, f in (("osm", step_osm), ("unet", step_unet)) if a.only in ("both", n)]
    if a.profile_steps:
        for _ in range(a.profile_steps):
            for _, f in legs:
                f()
        torch.cuda.synchronize()
        print(json.dumps({"profile_steps": a.profile_steps, "legs": [n for n, _ in legs]}))
        return
    for _ in range(a.warmup):
        for _, f in legs:
            f()
    torch.cuda.synchronize()
    blocks = {n: [] for n, _ in legs}
    for _ in range(a.blocks):
        for n, f in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                f()
            e1.record()
            torch.cuda.synchronize()
            blocks[n].append(e0.elapsed_time(e1) / a.steps)
    out = {"mode": a.mode, "x": list(x.shape), "osm_objs": list(objs.shape), "warmup": a.warmup, "steps_per_block": a.steps, "hip_graph": False}
    for n, b in blocks.items():
        out[n] = {"block_ms": [round(v, 4) for v in b], "median_ms": round(statistics.median(b), 4), "min_ms": round(min(b), 4),
                  "max_ms": round(max(b), 4)}
    if len(blocks) == 2:
        out["osm_minus_unet_ms"] = round(out["osm"]["median_ms"] - out["unet"]["median_ms"], 4)
        out["unet_block_spread_ms"] = round(out["unet"]["max_ms"] - out["unet"]["min_ms"], 4)
    oplan = next(iter(osm._oplans.values()))
    out["object_branch_calls"] = {"fwd": len(list(oplan.fwd.flat_calls())), "bwd": len(list(oplan.backward_plan(True, True).flat_calls()))}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
