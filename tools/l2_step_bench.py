"""Step time of L2Model (SRCNN, HighResNet) at the shipped option files' shape: B = 32, 8 revisits, 32 x 32 tiles, hidden 128, fp32.

    python tools/l2_step_bench.py [--arch SRCNN|HighResNet|both] [--batch 32] [--warmup 3] [--blocks 6] [--steps 8] [--cpu]
    python tools/l2_step_bench.py --arch SRCNN --profile-steps 3        # a short run for a kernel trace (no timing)

GPU: warm-up steps, then `blocks` timed blocks of `steps` optimize_parameters() calls each, every block between two device events;
prints the per-block milliseconds per step, their median and their spread.  --cpu: the CPU statement (l2_reference.py: forward with
random dropout masks, loss, backward through autograd) for the same step on this machine's torch threads, no optimizer - the same
work the device path replaces.  One JSON line per architecture."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def options(arch: str):
    opts = json.load(open(os.path.join(ROOT, "tests", "golden", "ssr_options.json")))
    name = {"SRCNN": "srcnn_s2naip_urban.yml", "HighResNet": "highresnet_s2naip_urban.yml"}[arch]
    return dict(opts[name], is_train=True, dist=False, path={})


def batch(B: int, R: int):
    g = torch.Generator().manual_seed(0)
    return {"lr": torch.randint(0, 256, (B, R, 3, 32, 32), generator=g, dtype=torch.uint8),
            "hr": torch.randint(0, 256, (B, 3, 128, 128), generator=g, dtype=torch.uint8)}


def gpu_leg(arch, a):
    from satlas_super_resolution_amd import models  # noqa: F401
    from satlas_super_resolution_amd.registry import build_model
    opt = options(arch)
    model = build_model(opt)
    data = batch(a.batch, opt["network_g"]["revisits"])
    model.update_learning_rate(1)
    model.feed_data(data)
    it = 0
    if a.profile_steps:
        for _ in range(a.profile_steps):
            it += 1
            model.optimize_parameters(it)
        torch.cuda.synchronize()
        return {"arch": arch, "profile_steps": a.profile_steps, "log": model.get_current_log()}
    for _ in range(a.warmup):
        it += 1
        model.optimize_parameters(it)
    torch.cuda.synchronize()
    blocks = []
    for _ in range(a.blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            it += 1
            model.optimize_parameters(it)
        e1.record()
        torch.cuda.synchronize()
        blocks.append(e0.elapsed_time(e1) / a.steps)
    log = model.get_current_log()
    n_launch = len(list(model.plan.fwd.flat_calls())) + len(list(model.plan.bwd.flat_calls()))
    return {"arch": arch, "batch": a.batch, "dtype": "fp32", "hip_graph": False, "warmup": a.warmup, "steps_per_block": a.steps,
            "block_ms_per_step": [round(b, 4) for b in blocks], "median_ms": round(statistics.median(blocks), 4),
            "min_ms": round(min(blocks), 4), "max_ms": round(max(blocks), 4), "images_per_s": round(a.batch * 1000 / statistics.median(blocks), 1),
            "plan_calls": n_launch, "log": {k: round(v, 6) for k, v in log.items()}, "skipped": model.nonfinite_skips}


def cpu_leg(arch, a):
    from satlas_super_resolution_amd import l2_reference as R
    from satlas_super_resolution_amd.models.ssr_l2_model import validate_options
    opt = options(arch)
    net = validate_options(opt)[0]
    kw = opt["network_g"]
    sd = {k: v.detach().clone().requires_grad_(v.numel() > 0) for k, v in net.state_dict().items()}
    data = batch(a.batch, kw["revisits"])
    x, gt = data["lr"].float() / 255, data["hr"].float() / 255
    fn = R.srcnn_reference if arch == "SRCNN" else R.highresnet_reference
    shapes = R.dropout_site_shapes(arch, a.batch, kw["revisits"], 32, 32, kw["hidden_channels"], kw["residual_layers"])
    times = []
    for _ in range(a.cpu_steps + 1):
        masks = [torch.rand(s) < 0.5 for s in shapes]
        t0 = time.perf_counter()
        out = fn(sd, x, masks)
        loss = R.l2_loss_reference(out.squeeze(1), gt)["tot_loss"]
        loss.backward()
        times.append((time.perf_counter() - t0) * 1000)
        for v in sd.values():
            v.grad = None
    return {"arch": arch, "what": "CPU statement, forward + loss + backward", "batch": a.batch, "torch_threads": torch.get_num_threads(),
            "first_ms": round(times[0], 1), "step_ms": [round(t, 1) for t in times[1:]], "median_ms": round(statistics.median(times[1:] or times), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="both")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--cpu-steps", type=int, default=2)
    ap.add_argument("--profile-steps", type=int, default=0)
    a = ap.parse_args()
    for arch in (("SRCNN", "HighResNet") if a.arch == "both" else (a.arch,)):
        print(json.dumps(cpu_leg(arch, a) if a.cpu else gpu_leg(arch, a)), flush=True)


if __name__ == "__main__":
    main()
