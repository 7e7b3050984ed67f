"""GPU: csrc/obj_crop.hip through the C ABI (ssr_obj_crop_resize_fwd / _bwd) against the float64 statement of
satlas_super_resolution_amd/osm_reference.py (crop_resize_reference / crop_resize_backward).

Scenes: images [2, 40, 40, 8] and [1, 128, 128, 8] (NHWC, junk in channels 3..7), and the 40 x 40 pair again as a 3-channel buffer
(the kernel's scalar read path).  Boxes: 1 x 1, 1 x 40, 40 x 1, 40 x 40, 33 x 31, 32 x 32, a 2 x 2 at each corner, two overlapping boxes in
one image, 128 x 128, 127 x 5, and an image with no object at all.  Both antialias settings.
Bound: the project's exact-fp32 gate, 2e-6 * max|reference| (README, "exact forms"): the forward is an FMA chain of at most 8 + 8
terms with weights that sum to 1, the backward sums at most 32 terms per row and 32 rows.
Adjoint identity <fwd(x), g> = <x, bwd(g)>, both sides evaluated in float64 from the DEVICE results: every device element is within
2e-6 * max|ref| of its exact value and the exact sides are equal, so the two differ by at most
2e-6 * (max|crops| * sum|g| + max|bwd| * sum|x|) - the same gate carried through the two inner products."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

GATE = 2e-6
SENT = 0x7FC5A5A5          # a NaN pattern: whatever a kernel leaves unwritten shows

BOXES_40 = [(0, 5, 7, 6, 8), (0, 9, 0, 10, 40), (0, 0, 0, 40, 40), (0, 3, 4, 36, 35), (0, 4, 6, 36, 38),
            (0, 0, 0, 2, 2), (0, 38, 0, 40, 2), (0, 0, 38, 2, 40), (0, 38, 38, 40, 40),
            (1, 5, 5, 25, 20), (1, 15, 10, 39, 33), (1, 0, 39, 40, 40)]
BOXES_128 = [(0, 0, 0, 128, 128), (0, 1, 60, 128, 65), (0, 20, 30, 52, 62)]
BOXES_LONELY = [(1, 2, 3, 30, 12), (1, 10, 8, 13, 40)]          # image 0 has no object
SCENES = {"40": ((2, 40, 40), 8, BOXES_40), "128": ((1, 128, 128), 8, BOXES_128), "lonely": ((2, 40, 40), 8, BOXES_LONELY),
          "40c3": ((2, 40, 40), 3, BOXES_40)}


def _hip():
    from satlas_super_resolution_amd import hip
    return hip, hip.lib()


def _ref():
    from satlas_super_resolution_amd import osm_reference
    return osm_reference


def _first(boxes, B):
    first = [0] * (B + 1)
    for b in range(B):
        first[b + 1] = first[b] + sum(1 for q in boxes if q[0] == b)
    return first


@functools.lru_cache(maxsize=None)
def scene(name, antialias):
    """inputs and float64 references of one scene, computed once and shared (never modified) by the tests"""
    (B, H, W), cs, boxes = SCENES[name]
    g = torch.Generator().manual_seed(1234 + len(name))
    img = torch.randn(B, H, W, cs, generator=g)                      # channels 3.. are junk the kernel must not read into the crop
    gout = torch.randn(len(boxes), 32, 32, 8, generator=g)
    base = 0.1 * torch.randn(B, H, W, cs, generator=g)               # what the image gradient holds before the backward
    R = _ref()
    x64 = img[..., :3].permute(0, 3, 1, 2).double()
    crops = R.crop_resize_reference(x64, boxes, antialias)                                                   # [Bo, 3, 32, 32]
    dimg = R.crop_resize_backward(gout[..., :3].permute(0, 3, 1, 2).double(), boxes, (B, 3, H, W), antialias)
    covered = torch.zeros(B, H, W, dtype=torch.bool)
    for b, x1, y1, x2, y2 in boxes:
        covered[b, y1:y2, x1:x2] = True
    return dict(B=B, H=H, W=W, cs=cs, boxes=boxes, img=img, gout=gout, base=base, crops=crops, dimg=dimg, covered=covered)


def run_fwd(s, antialias, boxes=None):
    hip, L = _hip()
    boxes = s["boxes"] if boxes is None else boxes
    img = s["img"].cuda()
    bx = torch.tensor(boxes, dtype=torch.int32).cuda()
    dst = torch.zeros(len(boxes), 32, 32, 8, dtype=torch.float32, device="cuda")
    dst.view(torch.int32).fill_(SENT)
    hip.check(L.ssr_obj_crop_resize_fwd(hip.View(img.data_ptr(), s["cs"], 0), hip.F32, s["B"], s["H"], s["W"], bx.data_ptr(), len(boxes),
                                        hip.View(dst.data_ptr(), 8, 0), int(antialias), hip.stream_ptr()), "ssr_obj_crop_resize_fwd")
    torch.cuda.synchronize()
    return dst.cpu()


def run_bwd(s, antialias, boxes=None, base=None, grad_scale=1.0):
    hip, L = _hip()
    boxes = s["boxes"] if boxes is None else boxes
    bx = torch.tensor(boxes, dtype=torch.int32).cuda()
    first = torch.tensor(_first(boxes, s["B"]), dtype=torch.int32).cuda()
    gout = s["gout"][:len(boxes)].contiguous().cuda()
    d = (s["base"] if base is None else base).clone().cuda()
    hip.check(L.ssr_obj_crop_resize_bwd(hip.View(gout.data_ptr(), 8, 0), bx.data_ptr(), first.data_ptr(), len(boxes),
                                        hip.View(d.data_ptr(), s["cs"], 0), hip.F32, s["B"], s["H"], s["W"], grad_scale, int(antialias),
                                        hip.stream_ptr()), "ssr_obj_crop_resize_bwd")
    torch.cuda.synchronize()
    return d.cpu()


def bits(t):
    return t.contiguous().view(torch.int32)


CASES = [(n, aa) for n in SCENES for aa in (False, True)]


@pytest.mark.parametrize("name,antialias", CASES)
def test_forward_against_float64(name, antialias):
    s = scene(name, antialias)
    out = run_fwd(s, antialias)
    ref = s["crops"].permute(0, 2, 3, 1)
    err = float((out[..., :3].double() - ref).abs().max())
    bound = GATE * float(ref.abs().max())
    print(f"obj_crop fwd {name} aa={antialias}: max err {err:.3e} bound {bound:.3e}")
    assert err <= bound
    assert bool((bits(out[..., 3:]) == 0).all()), "destination channels 3..7 are written as +0"


@pytest.mark.parametrize("antialias", (False, True))
def test_identity_size_returns_the_crop_bit_for_bit(antialias):
    for name, k in (("40", 4), ("128", 2)):
        s = scene(name, antialias)
        b, x1, y1, x2, y2 = s["boxes"][k]
        assert (x2 - x1, y2 - y1) == (32, 32)
        out = run_fwd(s, antialias)
        assert torch.equal(bits(out[k, :, :, :3]), bits(s["img"][b, y1:y2, x1:x2, :3]))


@pytest.mark.parametrize("name,antialias", CASES)
def test_backward_against_float64(name, antialias):
    s = scene(name, antialias)
    scale = 0.75
    d = run_bwd(s, antialias, grad_scale=scale)
    base, cov = s["base"], s["covered"]
    ref = base[..., :3].double() + scale * s["dimg"].permute(0, 2, 3, 1)
    err = float((d[..., :3].double() - ref).abs().max())
    bound = GATE * float((scale * s["dimg"]).abs().max())
    print(f"obj_crop bwd {name} aa={antialias}: max err {err:.3e} bound {bound:.3e}")
    assert err <= bound
    assert torch.equal(bits(d[..., 3:]), bits(base[..., 3:])), "channels >= 3 are left as they were"
    assert torch.equal(bits(d[~cov]), bits(base[~cov])), "pixels outside every box are left as they were"
    assert not torch.equal(bits(d[cov][:, :3]), bits(base[cov][:, :3]))


@pytest.mark.parametrize("name,antialias", [("40", False), ("40", True), ("128", True)])
def test_adjoint_identity(name, antialias):
    s = scene(name, antialias)
    crops = run_fwd(s, antialias)[..., :3].double()
    back = run_bwd(s, antialias, base=torch.zeros_like(s["base"]))[..., :3].double()
    g, x = s["gout"][..., :3].double(), s["img"][..., :3].double()
    lhs, rhs = float((crops * g).sum()), float((x * back).sum())
    bound = GATE * (float(s["crops"].abs().max()) * float(g.abs().sum()) + float(s["dimg"].abs().max()) * float(x[s["covered"]].abs().sum()))
    print(f"obj_crop adjoint {name} aa={antialias}: <fwd x, g> {lhs:.9e} <x, bwd g> {rhs:.9e} bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


def test_two_runs_give_the_same_bytes():
    s = scene("40", True)
    assert torch.equal(bits(run_fwd(s, True)), bits(run_fwd(s, True)))
    assert torch.equal(bits(run_bwd(s, True)), bits(run_bwd(s, True)))


def test_refused_boxes_give_zero_crops_and_no_gradient():
    s = scene("40", False)
    bad = [(0, 5, 5, 5, 9),        # empty
           (0, 30, 2, 41, 9),      # past the right edge
           (0, -1, 2, 8, 9),       # negative
           (0, 2, 30, 8, 41),      # past the bottom edge
           (2, 0, 0, 8, 8),        # no such image
           (-1, 0, 0, 8, 8),
           (1, 9, 9, 3, 12)]       # x2 < x1
    out = run_fwd(s, False, boxes=bad)
    assert bool((bits(out) == 0).all())
    d = run_bwd(s, False, boxes=bad)
    assert torch.equal(bits(d), bits(s["base"]))
    # a side above the cap (hip.OBJ_MAX_SIDE) is refused the same way; a box of exactly the cap is served (scene "128")
    hip, _ = _hip()
    big = dict(s, B=1, H=4, W=hip.OBJ_MAX_SIDE + 1, cs=8, img=torch.randn(1, 4, hip.OBJ_MAX_SIDE + 1, 8),
               base=torch.ones(1, 4, hip.OBJ_MAX_SIDE + 1, 8))
    wide = [(0, 0, 0, hip.OBJ_MAX_SIDE + 1, 4)]
    assert bool((bits(run_fwd(big, True, boxes=wide)) == 0).all())
    assert torch.equal(bits(run_bwd(big, True, boxes=wide)), bits(big["base"]))


def test_an_object_filed_under_another_image_gets_no_gradient():
    """`first` groups the objects by image; a box whose own image index disagrees with its group is skipped, not misapplied"""
    hip, L = _hip()
    s = scene("40", False)
    boxes = [(1, 2, 2, 20, 20)]
    bx = torch.tensor(boxes, dtype=torch.int32).cuda()
    first = torch.tensor([0, 1, 1], dtype=torch.int32).cuda()           # filed under image 0
    gout = s["gout"][:1].contiguous().cuda()
    d = s["base"].clone().cuda()
    hip.check(L.ssr_obj_crop_resize_bwd(hip.View(gout.data_ptr(), 8, 0), bx.data_ptr(), first.data_ptr(), 1, hip.View(d.data_ptr(), 8, 0),
                                        hip.F32, 2, 40, 40, 1.0, 0, hip.stream_ptr()), "ssr_obj_crop_resize_bwd")
    torch.cuda.synchronize()
    assert torch.equal(bits(d.cpu()), bits(s["base"]))
