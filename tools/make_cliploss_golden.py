"""Records tests/golden/cliploss_siglip_tiny.pt on the CPU: the `transformers` package's SiglipVisionModel (an independent plain-torch
statement of the tower) at the two tiny sizes of tests/cliploss_fixture.py, loaded with the rule-filled weights, run in float64 on
what clip_loss.clip_loss_input feeds a tower; the loss and its image gradient come from autograd through the package's model.

    python tools/make_cliploss_golden.py

Per case (tower x image size): the image seed, the inputs (uint8 k for float32 values k / 255), l_clip_sim, d l_clip_sim / d fake, and the sign margin min|fx - fg| /
max|fx|.  Only inputs and results are stored, no weights.  The image seed of a case is the first one from 0 whose sign margin is at
least cliploss_fixture.SIGN_MARGIN, so that no sign(fx - fg) can flip under fp32 rounding.  The project's own float64 definition
(clip_loss.clip_loss_reference under autograd) must agree with the package to 1e-9 max|ref| (asserted here, and again by
tests/test_clip_loss_host.py on what it loads)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def package_loss(model, fake64, gt64, size, weight):
    from satlas_super_resolution_amd import clip_loss as CL
    fake64 = fake64.clone().requires_grad_(True)
    fx = model(pixel_values=CL.clip_loss_input(fake64, size, torch.float64)).pooler_output
    with torch.no_grad():
        fg = model(pixel_values=CL.clip_loss_input(gt64, size, torch.float64)).pooler_output
    loss = weight * (fx - fg).abs().mean()
    loss.backward()
    margin = float((fx - fg).detach().abs().min() / fx.detach().abs().max())
    return loss.detach(), fake64.grad, margin


def main():
    import transformers
    import clipscore_fixture as FX
    import cliploss_fixture as LF
    from satlas_super_resolution_amd import clip_loss as CL
    from satlas_super_resolution_amd import clipscore_metric as CM
    out = {"loss_weight": LF.LOSS_WEIGHT, "towers": dict(LF.TOWERS), "tower_seed": dict(LF.TOWER_SEED), "cases": {},
           "transformers": transformers.__version__, "torch": torch.__version__}
    for name in LF.TOWERS:
        sd = LF.tower_state(name)
        size = CM.vit_config_from_state(sd)["image_size"]
        model = FX.hf_model("siglip", sd)
        for p in model.parameters():
            p.requires_grad_(False)
        for h, w in LF.SIZES:
            for seed in range(512):
                fake_u8, gt_u8 = LF.images(seed, h, w)
                fake, gt = LF.to_float(fake_u8), LF.to_float(gt_u8)
                loss, grad, margin = package_loss(model, fake.double(), gt.double(), size, LF.LOSS_WEIGHT)
                if margin >= LF.SIGN_MARGIN:
                    break
            else:
                raise SystemExit(f"{name} {h}x{w}: no image seed below 512 gives the sign margin")
            f = fake.double().requires_grad_(True)
            ours = CL.clip_loss_reference(f, gt.double(), sd, LF.LOSS_WEIGHT, "tanh", torch.float64)
            ours.backward()
            dl = abs(float(ours.detach() - loss)) / abs(float(loss))
            dg = float((f.grad - grad).abs().max() / grad.abs().max())
            assert dl <= 1e-9 and dg <= 1e-9, (name, h, w, dl, dg)
            out["cases"][LF.case_key(name, h, w)] = {"seed": seed, "fake_u8": fake_u8, "gt_u8": gt_u8, "loss": loss, "grad": grad, "margin": margin}
            print(f"{name} {h}x{w}: seed {seed}, loss {float(loss):.6f}, max|grad| {float(grad.abs().max()):.3e}, sign margin {margin:.2e}, "
                  f"own reference within {dl:.1e} (loss) {dg:.1e} (gradient)")
    torch.save(out, LF.PATH)
    print(LF.PATH, os.path.getsize(LF.PATH), "bytes")


if __name__ == "__main__":
    main()
