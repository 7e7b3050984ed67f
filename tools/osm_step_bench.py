"""Train-step time of OSMObjESRGANModel's step beside SSRESRGANModel's at the shape of osm_obj_esrgan.yml.

    python tools/osm_step_bench.py [--mode fp32h] [--warmup 3] [--blocks 6] [--steps 8]
    python tools/osm_step_bench.py --rocprof DIR [--profile-steps 3]       # + a serial kernel trace of its own for the two crop kernels
    python tools/osm_step_bench.py --profile-steps 3                      # what the trace runs: eager, one stream, no timing

B 16, 8 x Sentinel-2 TCI (24 input channels, 32 x 32), HR 128 x 128, the full generator (23 blocks, 64 features), D with num_feat 64 and
feed_disc_lr (27 input channels), n_osm_objs 1, random boxes of 2..128 pixels a side, new ones before every step.  One process; the two
steps ALTERNATE in blocks (A B A B ...) of `steps` graph replays between two device events - the object step's blocks include the
upload of the next boxes.  The baseline is the existing step, never the new code against itself: reported is the difference of the
two medians beside the spread of the baseline's own blocks.

--rocprof DIR starts `rocprofv3 --kernel-trace --stats` over a FRESH child process running `--profile-steps` (SSR_OVERLAP_D=0, no
graph: the launches in one stream, one after the other) and reports the rows of obj_crop_fwd_kernel / obj_crop_bwd_kernel from its
kernel_stats.csv, which is copied to DIR.  Not part of bench.py; one JSON line."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import random
import shutil
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

G_KW = dict(num_in_ch=24, num_out_ch=3, scale=4, num_feat=64, num_block=23, num_grow_ch=32)
D_KW = dict(num_in_ch=27, num_feat=64, skip_connection=True)


def random_boxes(rng, B, n, H, W):
    out = []
    for b in range(B):
        for _ in range(n):
            w, h = rng.randint(2, min(W, 128)), rng.randint(2, min(H, 128))
            x1, y1 = rng.randint(0, W - w), rng.randint(0, H - h)
            out.append((b, x1, y1, x1 + w, y1 + h))
    return out


def build_steps(a, which):
    import torch
    from satlas_super_resolution_amd.archs.osm_obj_discriminator_arch import OSMObjDiscriminator
    from satlas_super_resolution_amd.archs.rrdbnet_arch import SSR_RRDBNet
    from satlas_super_resolution_amd.osm_train_step import OSMObjTrainStep
    from satlas_super_resolution_amd.train_step import ESRGANTrainStep, StepConfig
    torch.manual_seed(0)
    cfg = StepConfig(feed_disc_lr=True, ema_decay=0.999)
    g_sd = SSR_RRDBNet(**G_KW).state_dict()
    d_net = OSMObjDiscriminator(**D_KW)
    with torch.no_grad():              # gamma = 0 is the initial value; any other costs the same
        d_net.o_attention1.gamma.fill_(0.7)
        d_net.o_attention2.gamma.fill_(-0.4)
    d_sd = d_net.state_dict()
    gen = torch.Generator().manual_seed(1)
    lr = torch.randint(0, 256, (a.batch, 24, 32, 32), generator=gen).float().cuda()
    hr = torch.randint(0, 256, (a.batch, 3, 128, 128), generator=gen).float().cuda()
    graph = not a.profile_steps
    steps = {}
    if which in ("both", "osm"):
        ts = OSMObjTrainStep(G_KW, D_KW, a.batch, 32, 32, a.mode, cfg, n_osm_objs=a.objs, osm_obj_weight=0.3, antialias=a.antialias,
                             use_graph=graph)
        ts.load_state(g_sd, d_sd)
        steps["osm"] = ts
    if which in ("both", "base"):
        ts = ESRGANTrainStep(G_KW, D_KW, a.batch, 32, 32, a.mode, cfg, use_graph=graph)
        ts.load_state(g_sd, d_sd)
        steps["base"] = ts
    for ts in steps.values():
        ts.feed_data(lr, hr, scale=1.0 / 255)
    return steps


def trace(a):
    """the serial kernel trace, in a child process of its own; returns the two kernels' rows"""
    os.makedirs(a.rocprof, exist_ok=True)
    tmp = os.path.join(a.rocprof, "trace_tmp")
    env = dict(os.environ, SSR_OVERLAP_D="0")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "k", "--", sys.executable, os.path.abspath(__file__),
           "--profile-steps", str(a.profile_steps or 3), "--mode", a.mode, "--batch", str(a.batch), "--objs", str(a.objs)] + (["--antialias"] if a.antialias else [])
    subprocess.run(cmd, check=True, env=env, stdout=subprocess.DEVNULL, timeout=900)
    found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if not found:
        raise SystemExit(f"no kernel_stats.csv under {tmp}")
    shutil.copy(found[0], os.path.join(a.rocprof, "kernel_stats.csv"))
    rows = [r for r in csv.DictReader(open(found[0])) if "obj_crop_" in r["Name"]]
    shutil.rmtree(tmp, ignore_errors=True)
    n = a.profile_steps or 3
    return {("fwd" if "fwd" in r["Name"] else "bwd"): {"calls_per_step": int(r["Calls"]) / n, "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                                                       "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
            for r in rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="fp32h")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--objs", type=int, default=1)
    ap.add_argument("--antialias", action="store_true")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--profile-steps", type=int, default=0)
    ap.add_argument("--rocprof", default=None)
    a = ap.parse_args()
    import torch
    rng = random.Random(0)
    if a.profile_steps and not a.rocprof:
        ts = build_steps(a, "osm")["osm"]
        for _ in range(a.profile_steps):
            ts.set_boxes(random_boxes(rng, a.batch, a.objs, 128, 128))
            ts.step()
        torch.cuda.synchronize()
        print(json.dumps({"profile_steps": a.profile_steps}))
        return
    kernels = trace(a) if a.rocprof else None          # (before this process opens the GPU)
    a.profile_steps = 0
    steps = build_steps(a, "both")

    def run(name):
        ts = steps[name]
        if name == "osm":
            ts.set_boxes(random_boxes(rng, a.batch, a.objs, 128, 128))
        ts.step()

    for _ in range(max(a.warmup, 2)):                  # (the second call captures the graph)
        for n in steps:
            run(n)
    torch.cuda.synchronize()
    blocks = {n: [] for n in steps}
    for _ in range(a.blocks):
        for n in steps:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                run(n)
            e1.record()
            torch.cuda.synchronize()
            blocks[n].append(e0.elapsed_time(e1) / a.steps)
    out = {"mode": a.mode, "batch": a.batch, "n_osm_objs": a.objs, "antialias": a.antialias, "warmup": a.warmup, "steps_per_block": a.steps,
           "hip_graph": True}
    for n, b in blocks.items():
        out[n] = {"block_ms": [round(v, 4) for v in b], "median_ms": round(statistics.median(b), 4), "min_ms": round(min(b), 4),
                  "max_ms": round(max(b), 4)}
    out["osm_minus_base_ms"] = round(out["osm"]["median_ms"] - out["base"]["median_ms"], 4)
    out["base_block_spread_ms"] = round(out["base"]["max_ms"] - out["base"]["min_ms"], 4)
    if kernels is not None:
        out["crop_kernels"] = kernels
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
