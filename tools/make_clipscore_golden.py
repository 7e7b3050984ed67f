"""Records tests/golden/clipscore_{siglip,clip}_tiny.pt on the CPU: the `transformers` package's SiglipVisionModel and
CLIPVisionModelWithProjection (independent plain-torch statements of the two towers) at the tiny sizes of tests/clipscore_fixture.py,
loaded with the rule-filled weights, run in float64 on what clipscore_metric.clip_resized_input feeds a tower.

    python tools/make_clipscore_golden.py

Each file: the uint8 inputs, per feed ('reference': BGR, raw [0, 1]; 'rgb+normalize') the features of every image and the scores of
the recorded pairs.  The project's own float64 reference must already agree with the package to 1e-9 max|ref| (asserted here, and
again by tests/test_clipscore_host.py on what it loads)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

FEEDS = {"reference": dict(bgr=True, normalize=False), "rgb+normalize": dict(bgr=False, normalize=True)}
PAIRS = ((0, 1), (0, 2), (1, 1))


def main():
    import transformers
    import clipscore_fixture as FX
    from satlas_super_resolution_amd import clipscore_metric as CM
    images = FX.fixture_images()
    for family in ("siglip", "clip"):
        sd = FX.tiny_state(family)
        cfg = CM.vit_config_from_state(sd)
        model = FX.hf_model(family, sd)
        out = {"family": family, "config": dict(FX.TINY[family]), "seed": FX.SEED[family], "images": images, "pairs": PAIRS,
               "features": {}, "scores": {}, "transformers": transformers.__version__, "torch": torch.__version__}
        for feed, kw in FEEDS.items():
            x = CM.clip_resized_input(images, cfg["image_size"], family, dtype=torch.float64, **kw)
            f = FX.hf_features(family, model, x)
            assert f.dtype == torch.float64 and f.shape == (images.shape[0], cfg["out_dim"])
            ours = CM.clip_image_features_reference(sd, images, gelu="tanh", **kw)
            dev = float((ours - f).abs().max() / f.abs().max())
            assert dev <= 1e-9, (family, feed, dev)
            out["features"][feed] = f
            out["scores"][feed] = torch.stack([CM.cosine_pairs_reference(f[i], f[j]) for i, j in PAIRS])
            print(f"{family} {feed}: max|f| {float(f.abs().max()):.3f}, own reference within {dev:.2e} max|ref|, scores {out['scores'][feed].tolist()}")
        path = os.path.join(FX.GOLDEN, f"clipscore_{family}_tiny.pt")
        torch.save(out, path)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
