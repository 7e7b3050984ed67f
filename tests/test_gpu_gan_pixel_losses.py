"""GPU: BasicSR's other pixel and GAN losses (csrc/losses.hip: ssr_pixel_loss, ssr_gan_loss) - the kernels through the C ABI against the
float64 statement of satlas_super_resolution_amd/gan_pixel_losses.py, their determinism and refusals, and the terms inside the train
step: against the oracle with the loss functions patched in, under graph replay, in deterministic mode and through the model plugin;
and that a default configuration still issues the launches it issued before.

Tolerance of the kernel tests (the scheme of tests/test_gpu_ssim_loss.py).  Every case computes e32, the error of the fp32 torch
statement against its float64 self on the same storage-rounded inputs, and holds the kernel to max(4 * e32, 1e-5 * max|ref|) - 4 for
another, equally valid fp32 summation order, the floor for cases where e32 happens to be tiny - after asserting that this bound is
within the project's gate of 1e-3 * max|ref|.  The piecewise-constant gradients of wgan and hinge are held to 2 ulp of fp32(+-w / n) and
to exactly 0 where the hinge is inactive; bf16 storage to one bf16 ulp of the rounded reference plus the fp32 bound.
With SSR_LOSS_VARIANTS_REPORT=<file> the observed figures are appended to that file (kept as
profiles/gan_pixel_losses/observed_errors.txt)."""
import json
import os

import pytest
import torch

from conftest import GOLDEN, parity_close, rel_err
from test_gpu_support_kernels import EINVAL, EUNSUP, Guarded, ibits, read_view, same_bits, strided

pytestmark = pytest.mark.gpu

SPAN = 1024                      # csrc/losses.hip: pixels per block the host sizes the grid with
CAP = 1024                       # ... and its cap on the blocks (SSR_LOSS_SLOTS = 256 under SSR_DETERMINISTIC)
PAST_CAP = CAP * SPAN + 5        # blocks walk more than once under either cap
SIZES = (1, 3, SPAN - 1, SPAN, SPAN + 1)
REAL, FAKE = 0.875, 0.125        # labels that are exact in bf16, so that "x == t" can be planted in both storage types
KINDS = (("MSELoss", 1e-12), ("CharbonnierLoss", 1e-12), ("CharbonnierLoss", 1e-6), ("CharbonnierLoss", 1e-2))
COMBOS = [(r, d) for r in (True, False) for d in (True, False)]      # (target_is_real, is_disc)
_REPORT = []


def note(line):
    _REPORT.append(line)
    print(line)


@pytest.fixture(scope="module", autouse=True)
def _report_file(request):
    yield
    path = os.environ.get("SSR_LOSS_VARIANTS_REPORT")
    if path and _REPORT:
        with open(path, "a") as f:
            f.write(f"# {request.module.__name__}\n" + "\n".join(_REPORT) + "\n")
        del _REPORT[:]


def _hip():
    from satlas_super_resolution_amd import hip
    return hip, hip.lib()


def _gp():
    from satlas_super_resolution_amd import gan_pixel_losses as GP
    return GP


def _bounds(l64, g64, e32_l, e32_g):
    """(loss bound, gradient bound)"""
    gmax, lmax = float(g64.abs().max()), abs(l64)
    bl, bg = max(4 * e32_l, 1e-5 * lmax), max(4 * e32_g, 1e-5 * gmax)
    assert bl <= 1e-3 * lmax and bg <= 1e-3 * gmax, "the inputs keep the derived bound under the project's gate"
    return bl, bg


def _check_grad(tag, got, g64, bg, mode, piecewise):
    """got, g64: float64 [npix, C]"""
    assert bool(torch.isfinite(got).all()), tag
    if mode == "bf16":
        from oracle.layerwise import bf16_ulp
        rr = g64.float().bfloat16().double()
        ulp = bf16_ulp(rr.abs().float()).double()
        bad = (got - rr).abs() > ulp * 1.0001 + bg
        bad |= (g64 == 0) & (got != 0)
        note(f"{tag} grad err / (bf16 ulp + bound) max {float(((got - rr).abs() / (ulp + bg)).max()):.3f}")
        assert not bool(bad.any()), (tag, float((got - rr).abs().max()))
    elif piecewise:
        r32 = g64.float().double()
        err = (got - r32).abs()
        note(f"{tag} grad err {float(err.max()):.3e} (2 ulp = {float((2 * 2.0 ** -23 * r32.abs()).max()):.3e})")
        assert bool((err <= 2 * 2.0 ** -23 * r32.abs()).all()), (tag, float(err.max()))      # where the reference is 0: exactly 0
    else:
        err = (got - g64).abs()
        note(f"{tag} grad err {float(err.max()):.3e} = {float(err.max()) / float(g64.abs().max()):.2e} max|g|  bound {bg:.3e}")
        assert bool((err <= bg).all()), (tag, float(err.max()), bg)


# ================================================================================================ ssr_pixel_loss
def _pixel_inputs(npix, c, seed):
    """uniform noise in [0, 1] with a region (the first third of the pixels) where a == b exactly: float64 [npix, C]"""
    g = torch.Generator().manual_seed(seed)
    a, b = torch.rand(npix, c, generator=g, dtype=torch.float64), torch.rand(npix, c, generator=g, dtype=torch.float64)
    b[:npix // 3] = a[:npix // 3]
    return a, b


def _pixel_reference(a, b, kind, weight, eps):
    """float64 loss and gradient, and the fp32 statement's own error against them: (l64, g64, e32_loss, e32_grad)"""
    GP = _gp()
    l64, g64 = GP.pixel_loss_grad_reference(a, b, kind, weight, eps)
    aa = a.float().requires_grad_(True)
    l32 = GP.pixel_loss_reference(aa, b.float(), kind, weight, eps)
    l32.backward()
    return float(l64), g64, abs(float(l32.detach()) - float(l64)), float((aa.grad.double() - g64).abs().max())


def _pixel_launch(va, vb, vg, code, npix, c, kind, eps, weight, loss_ptr):
    hip, L = _hip()
    return L.ssr_pixel_loss(va, vb, vg, code, npix, c, hip.PIXEL_KINDS.get(kind, kind), eps, weight, loss_ptr, hip.stream_ptr())


def _pixel_case(tag, npix, c, mode, lay, kind, eps, weight=0.7, flag=0):
    """one (size, layout, storage type, kind): the null-gradient form and the form with gradient"""
    hip, _ = _hip()
    code = hip.dtype_code(mode)
    tdt = hip.torch_dtype(code)
    a, b = _pixel_inputs(npix, c, seed=npix * 10 + c)
    a, b = a.to(tdt).double(), b.to(tdt).double()          # the float64 reference takes the storage-rounded inputs
    l64, g64, e32_l, e32_g = _pixel_reference(a, b, kind, weight, eps)
    bl, bg = _bounds(l64, g64, e32_l, e32_g)
    (acs, aco), (bcs, bco), (gcs, gco) = lay
    ga, va = strided(a, acs, aco, tdt)
    gb, vb = strided(b, bcs, bco, tdt)
    slots = hip.LOSS_SLOTS if flag else 1
    grid = min((npix + SPAN - 1) // SPAN, hip.LOSS_SLOTS) if flag else 1
    for form in ("null", "grad"):
        gl = Guarded(slots)
        gl.t[:grid] = 0.0
        gg = Guarded(npix * gcs, tdt) if form == "grad" else None          # the valid channels start as the NaN sentinel too
        vg = hip.View(gg.ptr(), gcs, gco) if gg is not None else hip.NULL_VIEW
        assert _pixel_launch(va, vb, vg, code | flag, npix, c, kind, eps, weight, gl.ptr()) == 0
        torch.cuda.synchronize()
        total = 0.0
        for v in gl.t[:grid].double().cpu().tolist():       # index order
            total += v
        el = abs(total - l64)
        note(f"{tag} {form:<4} loss err {el:.3e} bound {bl:.3e} (e32 {e32_l:.3e})")
        assert el <= bl, (tag, form, el, bl)
        assert gl.margins_intact() and ga.margins_intact() and gb.margins_intact()
        assert bool((ibits(gl.t)[grid:] == gl.sent).all())
        if gg is not None:
            _check_grad(tag, read_view(gg, gcs, gco, c).double(), g64, bg, mode, piecewise=False)
            assert gg.margins_intact() and gg.channels_intact(gcs, gco, c), "padding channels / guard bands of grad"
        assert ga.channels_intact(acs, aco, c) and gb.channels_intact(bcs, bco, c)
        assert torch.equal(read_view(ga, acs, aco, c).double(), a) and torch.equal(read_view(gb, bcs, bco, c).double(), b)


# C = 1 dense; three channels as aligned groups of four inside wider views (the train step's layout: whole-pixel loads); three channels
# at offsets that are no multiple of four (the per-channel path); seven channels - all three views laid out differently
PIXEL_LAYOUTS = [(1, ((1, 0), (8, 0), (4, 3))), (3, ((8, 0), (16, 4), (24, 9))), (3, ((16, 5), (24, 16), (16, 8))),
                 (7, ((8, 0), (8, 1), (16, 7)))]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("c,lay", PIXEL_LAYOUTS, ids=["C1", "C3-whole-pixel", "C3-offset", "C7"])
def test_pixel_loss_matches_float64(c, lay, mode):
    for npix in SIZES:
        for kind, eps in KINDS:
            _pixel_case(f"pixel {kind[:5]} eps {eps:g} {npix}x{c} {mode} {lay[0]}", npix, c, mode, lay, kind, eps)


@pytest.mark.parametrize("flag", [0, 0x200], ids=["default-cap", "deterministic-cap"])
def test_pixel_loss_past_the_grid_cap(flag):
    """more pixels than cap * span: every block walks its grid-stride loop more than once"""
    for kind, eps in KINDS[:2]:
        _pixel_case(f"pixel {kind[:5]} {PAST_CAP}x1 fp32 flag {flag:#x}", PAST_CAP, 1, "fp32", ((1, 0), (1, 0), (1, 0)), kind, eps, flag=flag)


# ================================================================================================ ssr_gan_loss
def _logits(npix, seed):
    """N(0, 3^2) with exact values planted: 0, +-1 (the hinge's kinks), the two labels (lsgan's zero) and +-100; float64 [npix, 1]"""
    g = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(npix, 1, generator=g, dtype=torch.float64)
    planted = torch.tensor([100.0, -100.0, 0.0, 1.0, -1.0, REAL, FAKE], dtype=torch.float64)
    if npix >= 3:
        k = min(npix, len(planted))
        x[:k, 0] = planted[:k]
    return x


def _gan_reference(x, gan_type, real, disc, weight):
    GP = _gp()
    l64, g64 = GP.gan_loss_grad_reference(x, gan_type, real, disc, weight, REAL, FAKE)
    xa = x.float().requires_grad_(True)
    l32 = GP.gan_loss_reference(xa, gan_type, real, disc, weight, REAL, FAKE)
    l32.backward()
    m64 = float(x.mean())
    return float(l64), g64, abs(float(l32.detach()) - float(l64)), float((xa.grad.double() - g64).abs().max()), m64, \
        abs(float(x.float().mean()) - m64)


def _gan_launch(vx, vg, code, npix, gan_type, real, disc, weight, loss_ptr, mean_ptr, target=None):
    hip, L = _hip()
    t = (REAL if real else FAKE) if target is None else target
    # the caller passes 1 for is_disc and loss_weight otherwise (GANLoss.forward), as the train step does
    return L.ssr_gan_loss(vx, vg, code, npix, hip.GAN_TYPES.get(gan_type, gan_type), int(real), int(disc), t, 1.0 if disc else weight,
                          loss_ptr, mean_ptr, hip.stream_ptr())


def _gan_case(tag, npix, mode, lay, gan_type, real, disc, weight=0.3, flag=0):
    hip, _ = _hip()
    code = hip.dtype_code(mode)
    tdt = hip.torch_dtype(code)
    x = _logits(npix, seed=npix).to(tdt).double()
    l64, g64, e32_l, e32_g, m64, e32_m = _gan_reference(x, gan_type, real, disc, weight)
    bl, bg = _bounds(l64, g64, e32_l, e32_g)
    # mean_out: the same scheme, with the floor at 1e-5 of what the signed terms add up from, mean|x| (mean(x) itself can cancel)
    bm = max(4 * e32_m, 1e-5 * float(x.abs().mean()))
    piecewise = gan_type in ("wgan", "hinge")
    (xcs, xco), (gcs, gco) = lay
    gx, vx = strided(x, xcs, xco, tdt)
    slots = hip.LOSS_SLOTS if flag else 1
    grid = min((npix + SPAN - 1) // SPAN, hip.LOSS_SLOTS) if flag else 1

    def read(gs):
        total = 0.0
        for v in gs.t[:grid].double().cpu().tolist():       # index order
            total += v
        return total
    for form in ("null", "grad"):
        gl, gm = Guarded(slots), Guarded(slots)
        gl.t[:grid] = 0.0
        gm.t[:grid] = 0.0
        gg = Guarded(npix * gcs, tdt) if form == "grad" else None
        vg = hip.View(gg.ptr(), gcs, gco) if gg is not None else hip.NULL_VIEW
        # the null-gradient form also leaves mean_out out
        assert _gan_launch(vx, vg, code | flag, npix, gan_type, real, disc, weight, gl.ptr(), gm.ptr() if gg is not None else None) == 0
        torch.cuda.synchronize()
        el = abs(read(gl) - l64)
        note(f"{tag} {form:<4} loss err {el:.3e} bound {bl:.3e} (e32 {e32_l:.3e})")
        assert el <= bl, (tag, form, el, bl)
        assert gl.margins_intact() and gm.margins_intact() and gx.margins_intact()
        assert bool((ibits(gl.t)[grid:] == gl.sent).all())
        if gg is None:
            continue
        em = abs(read(gm) - m64)
        note(f"{tag} mean err {em:.3e} bound {bm:.3e}")
        assert em <= bm, (tag, em, bm)
        _check_grad(tag, read_view(gg, gcs, gco, 1).double(), g64, bg, mode, piecewise)
        assert gg.margins_intact() and gg.channels_intact(gcs, gco, 1), "padding channels / guard bands of grad"
        assert gx.channels_intact(xcs, xco, 1) and torch.equal(read_view(gx, xcs, xco, 1).double(), x)


# dense; the train step's layout (channel 0 of 8); a non-zero offset of wider views, the two laid out differently
GAN_LAYOUTS = [((1, 0), (1, 0)), ((8, 0), (8, 0)), ((16, 5), (24, 9))]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("gan_type", ["lsgan", "wgan", "wgan_softplus", "hinge"])
def test_gan_loss_matches_float64(gan_type, mode):
    for lay in GAN_LAYOUTS:
        for npix in SIZES:
            for real, disc in COMBOS:
                _gan_case(f"gan {gan_type} real {int(real)} disc {int(disc)} {npix} {mode} {lay[0]}", npix, mode, lay, gan_type, real, disc)


@pytest.mark.parametrize("flag", [0, 0x200], ids=["default-cap", "deterministic-cap"])
def test_gan_loss_past_the_grid_cap(flag):
    for gan_type, real, disc in (("lsgan", True, False), ("wgan", False, True), ("wgan_softplus", True, True), ("hinge", False, True)):
        _gan_case(f"gan {gan_type} real {int(real)} disc {int(disc)} {PAST_CAP} fp32 flag {flag:#x}", PAST_CAP, "fp32", ((1, 0), (1, 0)),
                  gan_type, real, disc, flag=flag)


def test_fp32x3_storage_code_is_fp32():
    hip, _ = _hip()
    a, b = _pixel_inputs(77, 3, seed=1)
    ga, va = strided(a, 8, 0, torch.float32)
    gb, vb = strided(b, 8, 0, torch.float32)
    gx, vx = strided(_logits(77, seed=2), 8, 0, torch.float32)
    outs = []
    for code in (hip.F32, hip.F32X3):
        gg, g2, gl, gl2 = Guarded(77 * 8), Guarded(77 * 8), Guarded(1), Guarded(1)
        gl.t.zero_()
        gl2.t.zero_()
        assert _pixel_launch(va, vb, hip.View(gg.ptr(), 8, 0), code, 77, 3, "CharbonnierLoss", 1e-6, 0.7, gl.ptr()) == 0
        assert _gan_launch(vx, hip.View(g2.ptr(), 8, 0), code, 77, "hinge", True, True, 1.0, gl2.ptr(), None) == 0
        outs.append((gg, g2, gl, gl2))
    torch.cuda.synchronize()
    for p, q in zip(*outs):
        assert same_bits(p.buf, q.buf)


# ================================================================================================ determinism, refusals
@pytest.mark.parametrize("npix", [5 * SPAN + 1, 260 * SPAN + 3], ids=["6-blocks", "261-blocks"])
def test_determinism_and_loss_slots(npix):
    """the gradient has one writer per element: same bytes from two launches with and without SSR_DETERMINISTIC; under the flag block b
    is the single writer of slot b, the grid is min(blocks, SSR_LOSS_SLOTS) (261 blocks: some walk twice), the slots added in index
    order meet the loss bound, and a second launch doubles them"""
    hip, _ = _hip()
    a, b = _pixel_inputs(npix, 3, seed=11)
    a, b = a.float().double(), b.float().double()
    x = _logits(npix, seed=12).float().double()
    l64p, g64p, e32_l, e32_g = _pixel_reference(a, b, "MSELoss", 0.7, 0.0)
    blp, _ = _bounds(l64p, g64p, e32_l, e32_g)
    l64g, g64g, e32_l, e32_g, m64, e32_m = _gan_reference(x, "hinge", True, True, 1.0)
    blg, _ = _bounds(l64g, g64g, e32_l, e32_g)
    bm = max(4 * e32_m, 1e-5 * float(x.abs().mean()))
    ga, va = strided(a, 8, 0, torch.float32)
    gb, vb = strided(b, 8, 0, torch.float32)
    gx, vx = strided(x, 8, 0, torch.float32)
    grid = min((npix + SPAN - 1) // SPAN, hip.LOSS_SLOTS)
    runs = []
    for flag in (0, 0, hip.DETERMINISTIC, hip.DETERMINISTIC):
        n = hip.LOSS_SLOTS if flag else 1
        gp_, gg_ = Guarded(npix * 8), Guarded(npix * 8)
        sl = [Guarded(n) for _ in range(3)]
        for s in sl:
            s.t[:grid if flag else 1] = 0.0
        assert _pixel_launch(va, vb, hip.View(gp_.ptr(), 8, 0), hip.F32 | flag, npix, 3, "MSELoss", 0.0, 0.7, sl[0].ptr()) == 0
        assert _gan_launch(vx, hip.View(gg_.ptr(), 8, 0), hip.F32 | flag, npix, "hinge", True, True, 1.0, sl[1].ptr(), sl[2].ptr()) == 0
        torch.cuda.synchronize()
        assert all(s.margins_intact() for s in sl) and gp_.margins_intact() and gg_.margins_intact()
        runs.append((gp_, gg_, sl))
    for r in runs[1:]:
        assert same_bits(runs[0][0].buf, r[0].buf) and same_bits(runs[0][1].buf, r[1].buf)
    for s2, s3 in zip(runs[2][2], runs[3][2]):
        assert same_bits(s2.buf, s3.buf)
    for det, ref, bound, default, what in zip(runs[2][2], (l64p, l64g, m64), (blp, blg, bm), runs[0][2], ("pixel", "gan", "mean")):
        assert bool((ibits(det.t)[grid:] == det.sent).all()), "slots at and beyond the grid are untouched"
        total = 0.0
        for v in det.t[:grid].double().cpu().tolist():      # index order
            total += v
        note(f"det {what} slots ({grid} blocks, {npix} pixels) err {abs(total - ref):.3e} bound {bound:.3e}")
        assert abs(total - ref) <= bound and abs(float(default.t[0]) - ref) <= bound
    # `+=`: a second launch into the same slots doubles them (one writer per slot, launches on a stream are ordered)
    dp, dg, dm = runs[2][2]
    first = [s.t[:grid].clone() for s in (dp, dg, dm)]
    assert _pixel_launch(va, vb, hip.NULL_VIEW, hip.F32 | hip.DETERMINISTIC, npix, 3, "MSELoss", 0.0, 0.7, dp.ptr()) == 0
    assert _gan_launch(vx, hip.NULL_VIEW, hip.F32 | hip.DETERMINISTIC, npix, "hinge", True, True, 1.0, dg.ptr(), dm.ptr()) == 0
    torch.cuda.synchronize()
    for s, f in zip((dp, dg, dm), first):
        assert torch.equal(s.t[:grid], f + f)


def test_refusals_leave_outputs_untouched():
    hip, L = _hip()
    a, b = _pixel_inputs(4, 3, seed=1)
    ga, va = strided(a, 8, 0, torch.float32)
    gb, vb = strided(b, 8, 0, torch.float32)
    gx, vx = strided(_logits(4, seed=1), 8, 0, torch.float32)
    gg, gl, gm = Guarded(4 * 8), Guarded(1), Guarded(1)
    vg = hip.View(gg.ptr(), 8, 0)

    def pix(va_=va, code=hip.F32, npix=4, c=3, kind=1, eps=1e-12):
        return L.ssr_pixel_loss(va_, vb, vg, code, npix, c, kind, eps, 0.7, gl.ptr(), hip.stream_ptr())

    def gan(vx_=vx, code=hip.F32, npix=4, gt=4):
        return L.ssr_gan_loss(vx_, vg, code, npix, gt, 1, 1, 1.0, 1.0, gl.ptr(), gm.ptr(), hip.stream_ptr())
    assert pix(npix=0) == EINVAL and pix(c=0) == EINVAL and pix(c=9) == EINVAL and pix(va_=hip.View(None, 8, 0)) == EINVAL
    assert pix(eps=-1e-6) == EINVAL
    assert pix(kind=0) == EUNSUP and pix(kind=3) == EUNSUP and pix(code=7) == EUNSUP
    assert gan(npix=0) == EINVAL and gan(vx_=hip.View(None, 8, 0)) == EINVAL and gan(vx_=hip.View(gx.ptr(), 8, 8)) == EINVAL
    assert gan(gt=0) == EUNSUP and gan(gt=5) == EUNSUP and gan(code=7) == EUNSUP
    torch.cuda.synchronize()
    for g in (gg, gl, gm):
        assert bool((ibits(g.buf) == g.sent).all())


# ================================================================================================ the terms inside the train step
G_KW = dict(num_in_ch=6, num_out_ch=3, scale=4, num_feat=16, num_block=1, num_grow_ch=8)      # the tiny networks of tests/test_gpu_ssim_loss.py
D_KW = dict(num_in_ch=3, num_feat=8, skip_connection=True)
GAN_W = 5.0       # at the shipped gan_opt.loss_weight of 0.1 the adversarial term moves the tiny generator's gradients by 3e-3 .. 8e-3 only


def _urban():
    opt = json.load(open(os.path.join(GOLDEN, "ssr_options.json")))["esrgan_s2naip_urban.yml"]
    opt["feed_disc_lr"] = False
    del opt["train"]["perceptual_opt"]
    return opt


def _step_setup(gan=None, pixel=None):
    from oracle import esrgan_oracle as O
    from satlas_super_resolution_amd.models.ssr_esrgan_model import train_config_from_opt
    opt = _urban()
    opt["train"]["gan_opt"].update(gan or {})
    opt["train"]["pixel_opt"].update(pixel or {})
    cfg = train_config_from_opt(opt)
    g0, d0 = O.generator_init(seed=41, **G_KW), O.discriminator_init(3, 8, seed=42)
    torch.manual_seed(44)
    lr, gt = torch.rand(2, 6, 16, 16), torch.rand(2, 3, 64, 64)
    return cfg, g0, d0, lr, gt


def _oracle(cfg, g0, d0, lr, gt, monkeypatch=None, gan_type=None, pixel_type=None, labels=None):
    """one oracle step; with `monkeypatch`, the oracle's module-level l1_loss / gan_loss_vanilla are the reference functions of the
    given types (default: cfg's) for the duration of the test"""
    from oracle import esrgan_oracle as O
    GP = _gp()
    if monkeypatch is not None:
        gt_, pt_ = gan_type or cfg.gan_type, pixel_type or cfg.pixel_type
        rl, fl = labels or (cfg.real_label, cfg.fake_label)
        monkeypatch.setattr(O, "l1_loss", lambda pred, target, weight=1.0: GP.pixel_loss_reference(pred, target, pt_, weight, cfg.pixel_eps))
        monkeypatch.setattr(O, "gan_loss_vanilla", lambda pred, target_is_real, is_disc, loss_weight=0.1, real_label_val=1.0,
                            fake_label_val=0.0: GP.gan_loss_reference(pred, gt_, target_is_real, is_disc, loss_weight, rl, fl))
    ocfg = O.StepConfig(l1_weight=cfg.l1_weight, gan_weight=cfg.gan_weight, lr_g=cfg.lr_g, lr_d=cfg.lr_d, betas=cfg.betas,
                        ema_decay=cfg.ema_decay, l1_gt_usm=cfg.l1_gt_usm, gan_gt_usm=cfg.gan_gt_usm)
    orc = O.ESRGANOracle(g0, d0, ocfg)
    log = orc.step(lr, gt, 1)
    return orc, log


def _moved(a, b):
    """per tensor with a non-zero reference: the largest change as a fraction of the largest reference value"""
    return {k: float((a[k] - b[k]).abs().max() / a[k].abs().max()) for k in a if float(a[k].abs().max()) > 0}


def _device_step(cfg, g0, d0, lr, gt, mode="fp32", use_graph=False, iters=(1,)):
    from satlas_super_resolution_amd.train_step import ESRGANTrainStep
    B = lr.shape[0]
    ts = ESRGANTrainStep(G_KW, D_KW, B, 16, 16, mode, cfg, use_graph=use_graph)
    ts.load_state(g0, d0)
    ts.feed_data(lr.cuda(), gt.cuda())
    for it in iters:
        ts.step(it)
    return ts


def _compare_step(tag, ts, orc, ref_log):
    log = ts.log()
    assert set(log) == set(ref_log)
    for k, v in ref_log.items():
        note(f"{tag} {k} got {log[k]:.6e} ref {v:.6e}")
        assert abs(log[k] - v) <= 1e-3 * max(1.0, abs(v)), (k, log[k], v)
    for k, g in orc.g_grads.items():                       # the bounds of tests/test_gpu_ssim_loss.py
        got = ts.g_store.tensor(k, ts.g_store.grad)
        gc_, gr_ = got.detach().float().cpu(), g.detach().float().cpu()
        err, scale = (gc_ - gr_).abs(), float(gr_.abs().max())
        outside = int((err > 2e-3 * (scale + gr_.abs())).sum())
        assert outside <= max(3, int(2e-3 * err.numel())) and float(err.max()) <= 1e-2 * scale and float(err.mean()) <= 1e-3 * scale, \
            (k, outside, err.numel(), float(err.max()) / scale)
    for k, g in orc.d_grads.items():
        got = ts.d_store.tensor(k, ts.d_store.grad)
        if float(g.abs().max()) == 0.0:
            # a reference gradient that is identically zero (wgan / hinge: conv9.bias, whose contributions -1 and +1 of the real and the
            # fake pass cancel) offers no scale: held to an absolute 1e-3 of those contributions
            note(f"{tag} d grad {k}: reference identically 0, got max {float(got.abs().max()):.3e}")
            assert float(got.abs().max()) <= 1e-3, (k, float(got.abs().max()))
        else:
            assert parity_close(got, g), ("d grad", k, rel_err(got, g))


@pytest.mark.parametrize("gan_type", ["lsgan", "wgan", "hinge"])
def test_train_step_gan_types_match_the_patched_oracle(gan_type, monkeypatch):
    cfg, g0, d0, lr, gt = _step_setup(gan={"gan_type": gan_type, "loss_weight": GAN_W})
    assert cfg.gan_type == gan_type and cfg.gan_weight == GAN_W
    plain, _ = _oracle(cfg, g0, d0, lr, gt)
    orc, ref_log = _oracle(cfg, g0, d0, lr, gt, monkeypatch)
    # the term matters: gradients of both networks move by more than ten times the gate against the vanilla oracle
    mg, md = _moved(orc.g_grads, plain.g_grads), _moved(orc.d_grads, plain.d_grads)
    note(f"step {gan_type}: moved G max {max(mg.values()):.3f} min {min(mg.values()):.3f}, D max {max(md.values()):.3f}")
    assert max(mg.values()) > 10 * 2e-3 and max(md.values()) > 10 * 2e-3, (mg, md)
    ts = _device_step(cfg, g0, d0, lr, gt)
    _compare_step(f"step {gan_type}", ts, orc, ref_log)
    if gan_type in ("wgan", "hinge"):
        assert ref_log["l_g_gan"] < 0 and ts.log()["l_g_gan"] < 0      # -w * mean(D(G(x))) on positive logits: signed losses are logged as they are


@pytest.mark.parametrize("pixel", [{"type": "MSELoss"}, {"type": "CharbonnierLoss", "eps": 1e-2}], ids=["MSELoss", "Charbonnier-1e-2"])
def test_train_step_pixel_types_match_the_patched_oracle(pixel, monkeypatch):
    """Charbonnier at its default eps of 1e-12 differs from L1 by 2e-6 of the gradients: eps 1e-2 makes the term visible"""
    cfg, g0, d0, lr, gt = _step_setup(pixel=pixel)
    assert cfg.pixel_type == pixel["type"] and cfg.pixel_eps == pixel.get("eps", 1e-12) and cfg.gan_type == "vanilla"
    plain, _ = _oracle(cfg, g0, d0, lr, gt)
    orc, ref_log = _oracle(cfg, g0, d0, lr, gt, monkeypatch)
    mg = _moved(orc.g_grads, plain.g_grads)
    note(f"step {pixel['type']}: moved G max {max(mg.values()):.3f}")
    assert max(mg.values()) > 10 * 2e-3, mg
    ts = _device_step(cfg, g0, d0, lr, gt)
    _compare_step(f"step {pixel['type']}", ts, orc, ref_log)


def test_train_step_wgan_softplus_ignores_the_labels(monkeypatch):
    """wgan_softplus is vanilla at labels 1 / 0 whatever the label values say (GANLoss.get_target_label): with real_label_val 0.9 the
    step matches the UNPATCHED oracle, whose vanilla loss has labels 1 / 0 - which a vanilla loss at 0.9 does not"""
    cfg, g0, d0, lr, gt = _step_setup(gan={"gan_type": "wgan_softplus", "loss_weight": GAN_W, "real_label_val": 0.9})
    assert cfg.gan_type == "wgan_softplus" and cfg.real_label == 0.9
    plain, ref_log = _oracle(cfg, g0, d0, lr, gt)
    at09, _ = _oracle(cfg, g0, d0, lr, gt, monkeypatch, gan_type="vanilla")
    monkeypatch.undo()
    mg, md = _moved(plain.g_grads, at09.g_grads), _moved(plain.d_grads, at09.d_grads)
    note(f"step wgan_softplus: vanilla at 0.9 against 1.0 moves G max {max(mg.values()):.3f}, D max {max(md.values()):.3f}")
    assert max(mg.values()) > 10 * 2e-3 and max(md.values()) > 10 * 2e-3, (mg, md)
    ts = _device_step(cfg, g0, d0, lr, gt)
    _compare_step("step wgan_softplus", ts, plain, ref_log)


@pytest.mark.parametrize("gan,pixel", [({"gan_type": "hinge"}, None), (None, {"type": "CharbonnierLoss"})], ids=["gan-family", "pixel-family"])
def test_train_step_graph_replay(gan, pixel):
    cfg, g0, d0, lr, gt = _step_setup(gan=gan, pixel=pixel)
    ts = _device_step(cfg, g0, d0, lr, gt, use_graph=True, iters=(1, 2, 3))      # warm-up, capture, replay
    log = ts.log()
    assert set(log) == {"l_g_pix", "l_g_gan", "l_d_real", "out_d_real", "l_d_fake", "out_d_fake"}
    assert all(v == v and abs(v) != float("inf") for v in log.values()), log
    assert log["l_g_pix"] > 0


def test_hinge_and_mse_are_deterministic_in_fp32h():
    cfg, g0, d0, lr, gt = _step_setup(gan={"gan_type": "hinge"}, pixel={"type": "MSELoss"})
    cfg.deterministic = True
    lr, gt = lr.repeat(2, 1, 1, 1), gt.repeat(2, 1, 1, 1)
    runs = []
    for _ in range(2):
        ts = _device_step(cfg, g0, d0, lr, gt, mode="fp32h", use_graph=True, iters=(1, 2))
        log = ts.log()
        runs.append((tuple(log.values()), ts.output().cpu(), ts.g_store.data.detach().cpu().clone(), ts.d_store.data.detach().cpu().clone()))
    assert runs[0][0] == runs[1][0] and runs[0][0][0] > 0
    for p, q in zip(runs[0][1:], runs[1][1:]):
        assert torch.equal(p, q)


def test_model_plugin_runs_hinge_and_charbonnier(tmp_path, monkeypatch):
    from satlas_super_resolution_amd import models, perceptual as P  # noqa: F401
    from satlas_super_resolution_amd.registry import build_model
    opt = json.load(open(os.path.join(GOLDEN, "ssr_options.json")))["esrgan_s2naip_urban.yml"]
    opt.update(is_train=True, dist=False, rank=0, world_size=1, compute_dtype="fp32h")
    opt["path"].update(models=str(tmp_path / "models"), training_states=str(tmp_path / "states"), visualization=str(tmp_path / "vis"))
    opt["network_d"]["num_in_ch"] = 3 + opt["network_g"]["num_in_ch"]     # as in test_gpu_boundary: the shipped D width cannot run
    opt["network_g"]["num_block"] = 2                                     # the loss plumbing is under test, not the body's depth
    opt["train"]["gan_opt"]["gan_type"] = "hinge"
    opt["train"]["pixel_opt"]["type"] = "CharbonnierLoss"
    wfile = tmp_path / "vgg19-dcbb9e9d.pth"
    torch.save(P.vgg19_random_state(P.vgg19_specs("conv5_4"), seed=1), wfile)
    monkeypatch.setenv("SSR_VGG19_WEIGHTS", str(wfile))
    model = build_model(json.loads(json.dumps(opt)))
    assert (model.cfg.gan_type, model.cfg.pixel_type, model.cfg.pixel_eps) == ("hinge", "CharbonnierLoss", 1e-12)
    g = torch.Generator().manual_seed(0)
    for it in (1, 2):
        model.update_learning_rate(it, warmup_iter=-1)
        model.feed_data({"lr": torch.randint(0, 256, (2, 36, 32, 32), generator=g, dtype=torch.uint8),
                         "hr": torch.randint(0, 256, (2, 3, 128, 128), generator=g, dtype=torch.uint8)})
        model.optimize_parameters(it)
    log = model.get_current_log()
    assert set(log) == {"l_g_pix", "l_g_percep", "l_g_gan", "l_d_real", "out_d_real", "l_d_fake", "out_d_fake"}
    assert all(v == v and abs(v) != float("inf") for v in log.values()) and log["l_g_pix"] > 0 and log["l_d_real"] >= 0
    bad = json.loads(json.dumps(opt))
    bad["train"]["gan_opt"]["gan_type"] = "foo"
    with pytest.raises(NotImplementedError, match="gan_type"):
        build_model(bad)


# ================================================================================================ unchanged behaviour
class _Recorder:
    """hip.lib() with the name of every ssr_* call noted in order"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not name.startswith("ssr_"):
            return f

        def call(*a):
            self.calls.append(name)
            return f(*a)
        return call


def test_default_options_issue_the_same_calls_as_before(monkeypatch):
    """L1Loss + vanilla: neither new entry is called, ssr_l1_loss once and ssr_bce_logits_loss three times per step; hinge + MSELoss
    issues the same sequence with exactly those four calls replaced"""
    hip, L = _hip()
    rec = _Recorder(L)
    monkeypatch.setattr(hip, "lib", lambda: rec)
    seqs = {}
    for name, (gan, pixel) in {"default": (None, None), "variant": ({"gan_type": "hinge"}, {"type": "MSELoss"})}.items():
        cfg, g0, d0, lr, gt = _step_setup(gan=gan, pixel=pixel)
        ts = _device_step(cfg, g0, d0, lr, gt, iters=())
        for it in (1, 2):
            del rec.calls[:]
            ts.step(it)
            torch.cuda.synchronize()
            seqs[name, it] = list(rec.calls)
    for it in (1, 2):
        d, v = seqs["default", it], seqs["variant", it]
        assert d.count("ssr_l1_loss") == 1 and d.count("ssr_bce_logits_loss") == 3
        assert d.count("ssr_pixel_loss") == 0 and d.count("ssr_gan_loss") == 0
        assert v.count("ssr_pixel_loss") == 1 and v.count("ssr_gan_loss") == 3
        assert v.count("ssr_l1_loss") == 0 and v.count("ssr_bce_logits_loss") == 0
        swap = {"ssr_pixel_loss": "ssr_l1_loss", "ssr_gan_loss": "ssr_bce_logits_loss"}
        assert [swap.get(c, c) for c in v] == d
