"""Host wall time of building the two real-size tower plans, for the tree the script is started in (`cd <tree> && python
<this file> [label]`): the CLIP loss plan of a ViT-B/16-SigLIP-256-sized tower at B = 32, 128 x 128, and the CLIPScore metric plan of
an SO400M-sized tower at B = 2, 128 x 128, random weights.  Building a plan is host work done once per shape; each is built eight
times between device synchronisations, and the first (allocator warm-up), the median and maximum of the other seven and the minimum
are printed as one JSON line.  There is no CPU path: the figures are for the machine that runs the step."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from satlas_super_resolution_amd import clip_loss as CL, clipscore_metric as CM, hip  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("tools/tower_plan_build_time.py needs a GPU")
assert os.path.abspath(CL.__file__).startswith(os.getcwd()), CL.__file__
B, H, W = 32, 128, 128
loss_model = CL.ClipLossModel(CM.clip_random_state("siglip", seed=3, width=768, depth=12, mlp=3072, patch=16, grid=16, heads=12), "cuda")
images, grad, loss = torch.zeros(B, H, W, 8, device="cuda"), torch.zeros(B, H, W, 8, device="cuda"), torch.zeros(hip.LOSS_SLOTS, device="cuda")
metric_model = CM.CLIPVisualModel(CM.clip_random_state("siglip", seed=1), "cuda")
builders = {"loss_plan_vitb16_256_ms": lambda: CL.ClipLossPlan(loss_model, B, H, W, hip.View(images.data_ptr(), 8, 0), hip.View(images.data_ptr(), 8, 4),
                                                               hip.View(grad.data_ptr(), 8, 0), loss.data_ptr(), 0.5, hip.DETERMINISTIC),
            "metric_plan_so400m_ms": lambda: CM.CLIPVisualPlan(metric_model, 2, 128, 128)}
out = {"tree": sys.argv[1] if len(sys.argv) > 1 else os.getcwd()}
for name, build in builders.items():
    ms = []
    for _ in range(8):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan = build()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        calls = len(plan.launcher)
        del plan
    out[name] = {"first": round(ms[0], 3), "median_of_rest": round(statistics.median(ms[1:]), 3), "min": round(min(ms), 3),
                 "max_of_rest": round(max(ms[1:]), 3), "calls": calls}
print(json.dumps(out), flush=True)
