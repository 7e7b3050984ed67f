"""Host wall time of building the three backbone plans, for the tree the script is started in (`cd <tree> && python <this file>
[label]`): PerceptualPlan at the benchmark's shape (B = 32, 128 x 128, fp32h, the shipped layer_weights, random VGG19 weights) and
LPIPSModel.plan(32, 128, 128) for both backbones.  Building a plan is host work done once per shape; each is built eight times between
device synchronisations, and the first (allocator warm-up), the median and maximum of the other seven and the minimum are printed as
one JSON line.  There is no CPU path: the figures are for the machine that runs the step."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from satlas_super_resolution_amd import hip, lpips_metric as LM, perceptual as P  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("tools/backbone_plan_build_time.py needs a GPU")
assert os.path.abspath(P.__file__).startswith(os.getcwd()), P.__file__
B, H, W = 32, 128, 128
opt = {"type": "PerceptualLoss", "layer_weights": {"conv1_2": 0.1, "conv2_2": 0.1, "conv3_4": 1, "conv4_4": 1, "conv5_4": 1}, "vgg_type": "vgg19",
       "use_input_norm": True, "perceptual_weight": 1.0, "style_weight": 0, "range_norm": False, "criterion": "l1"}
state = P.vgg19_random_state(P.vgg19_specs("conv5_4"), seed=2)
x, tgt, grad = (torch.zeros(B, H, W, 8, device="cuda") for _ in range(3))
loss = torch.zeros(hip.LOSS_SLOTS, device="cuda")
models = {n: LM.LPIPSModel(LM.lpips_random_state(0, net=n), "cuda", net=n) for n in ("vgg", "alex")}


def lpips_plan(net):
    models[net].plans.clear()
    return models[net].plan(B, H, W).launcher


builders = {"perceptual_plan_ms": lambda: P.PerceptualPlan(opt, B, H, W, hip.F32H, x, tgt, grad, loss.data_ptr(), state=state).bwd,
            "lpips_vgg_plan_ms": lambda: lpips_plan("vgg"), "lpips_alex_plan_ms": lambda: lpips_plan("alex")}
out = {"tree": sys.argv[1] if len(sys.argv) > 1 else os.getcwd()}
for name, build in builders.items():
    ms = []
    for _ in range(8):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        launcher = build()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        calls = len(launcher)
        del launcher
    out[name] = {"first": round(ms[0], 3), "median_of_rest": round(statistics.median(ms[1:]), 3), "min": round(min(ms), 3),
                 "max_of_rest": round(max(ms[1:]), 3), "calls": calls}
print(json.dumps(out), flush=True)
