"""Time of the LPIPS validation metric (lpips_metric.lpips_distance: VGG16 forward in exact fp32 + csrc/lpips.hip) on one GPU, at
the validation image size: 1 x 128 x 128 (what `calculate_lpips` scores per call) and 32 x 128 x 128, with random weights of the
architecture.  Beside it: the psnr + ssim + cpsnr calls on the same images (one image per call, as validation runs them) and
lpips_reference in float32 on the host's cores.  Device times are HIP-event pairs around whole calls (the download of the partials
included), after a warm-up; medians, minima and maxima are printed as one JSON line.  There is no CPU path for the device legs.

  python tools/lpips_metric_time.py [--reps 30] [--warmup 5] [--threads 16]
  python tools/lpips_metric_time.py --trace     # under rocprofv3 --kernel-trace --stats (a run of its own): lpips_distance only
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "reps": reps}


def run(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/lpips_metric_time.py needs a GPU: the metric has no CPU path")
    from satlas_super_resolution_amd import lpips_metric as LM, metrics as M
    torch.set_num_threads(args.threads)
    state = LM.lpips_random_state(0)
    model = LM.LPIPSModel(state, "cuda")
    g = torch.Generator().manual_seed(0)
    out = {"what": "lpips_distance (VGG16 exact fp32 + csrc/lpips.hip), H = W = 128", "host_threads": args.threads}
    for n in (1, 32):
        a = torch.randint(0, 256, (n, 128, 128, 3), generator=g, dtype=torch.uint8)
        b = (a.int() + torch.randint(-8, 9, a.shape, generator=g, dtype=torch.int32)).clamp(0, 255).to(torch.uint8)
        ad, bd = a.cuda(), b.cuda()
        leg = {"lpips_distance": timed(lambda: LM.lpips_distance(ad, bd, model), 4 if args.trace else args.reps, 2 if args.trace else args.warmup)}
        if not args.trace:
            def three():
                for i in range(n):
                    M.calculate_psnr(ad[i:i + 1], bd[i:i + 1], 4)
                    M.calculate_ssim(ad[i:i + 1], bd[i:i + 1], 4)
                    M.calculate_cpsnr(ad[i:i + 1], bd[i:i + 1], 4)
            leg["psnr+ssim+cpsnr"] = timed(three, args.reps, args.warmup)
            cpu = []
            for _ in range(3):
                t0 = time.perf_counter()
                ref = LM.lpips_reference(a, b, state, dtype=torch.float32)
                cpu.append((time.perf_counter() - t0) * 1e3)
            leg["lpips_reference_fp32_host"] = {"median_ms": round(statistics.median(cpu), 2), "min_ms": round(min(cpu), 2),
                                                "max_ms": round(max(cpu), 2), "reps": 3}
            got = LM.lpips_distance(ad, bd, model)
            leg["device_vs_host_fp32_rel"] = float(((got - ref.double()).abs() / ref.double()).max())
        out[f"N={n}"] = leg
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--trace", action="store_true", help="few calls of lpips_distance only (for a kernel trace)")
    run(ap.parse_args())


if __name__ == "__main__":
    main()
