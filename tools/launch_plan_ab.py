"""Same-visit evidence that two trees of this project run the same train step (profiles/launch_plans/): for fp32, bf16, fp32x3 and
fp32h, three iterations of the tiny deterministic train step of tests/test_gpu_deterministic.py (B = 4, 32 x 32, 2 blocks,
`deterministic: true`), then the sha256 of both parameter arenas and of the loss slots.  Deterministic steps are bit-reproducible, so
two trees that launch the same kernels with the same arguments in the same order print the same lines.

  python tools/launch_plan_ab.py --root <tree> --out ab.txt           # needs the GPU; <tree> holds a built satlas_super_resolution_amd
  python tools/launch_plan_ab.py --root <tree> --build-time 5         # wall seconds of 5 ESRGANTrainStep(...) at the benchmark's shape
"""
import argparse
import hashlib
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out")
ap.add_argument("--build-time", type=int, default=0)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402
from oracle import esrgan_oracle as O  # noqa: E402
import satlas_super_resolution_amd  # noqa: E402
from satlas_super_resolution_amd.train_step import ESRGANTrainStep, StepConfig  # noqa: E402

assert os.path.abspath(satlas_super_resolution_amd.__file__).startswith(os.path.abspath(args.root) + os.sep), satlas_super_resolution_amd.__file__
G_KW = dict(num_in_ch=24, num_out_ch=3, scale=4, num_feat=64, num_block=2, num_grow_ch=32)
D_KW = dict(num_in_ch=3, num_feat=64, skip_connection=True)
B = 4


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def three_steps(mode):
    ts = ESRGANTrainStep(G_KW, D_KW, B, 32, 32, mode, StepConfig(deterministic=True), use_graph=False)
    ts.load_state(O.generator_init(seed=21, **G_KW), O.discriminator_init(3, 64, seed=22))
    g = torch.Generator().manual_seed(23)
    for it in range(1, 4):
        lr, gt = torch.rand(B, 24, 32, 32, generator=g), torch.rand(B, 3, 128, 128, generator=g)
        ts.feed_data(lr.cuda(), gt.cuda())
        ts.step(it)
    torch.cuda.synchronize()
    return f"{mode} g {digest(ts.g_store.data)} d {digest(ts.d_store.data)} losses {digest(ts.losses)}"


def build_times(n):
    """wall seconds of each of n constructions of the benchmark's train step (bench.py defaults: fp32h, B = 32, 23 blocks); one
    construction before them loads the library and initialises the device"""
    g_kw, out = dict(G_KW, num_block=23), []
    for i in range(n + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ts = ESRGANTrainStep(g_kw, D_KW, 32, 32, 32, "fp32h", StepConfig(deterministic=True), use_graph=True)
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
        del ts
    return out[1:]


if args.build_time:
    print("ESRGANTrainStep build seconds:", " ".join("%.3f" % t for t in build_times(args.build_time)))
else:
    lines = [three_steps(m) for m in ("fp32", "bf16", "fp32x3", "fp32h")]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
