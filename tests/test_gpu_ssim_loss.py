"""GPU: the SSIM loss of train.ssim_opt (csrc/ssim.hip, ssr_ssim_loss) - the kernel through the C ABI against the float64 statement
of satlas_super_resolution_amd/ssim_loss.py, its determinism and refusals, and the term inside the train step: against the oracle
with the term patched in, without perceptual_opt, in deterministic mode, and through the model plugin.

Tolerance of the kernel tests.  The usual 1e-4 of max|ref| is not the measure here: the reference's own fp32 arithmetic misses it
(E[x^2] - E[x]^2 against C2 = 9e-4 in flat regions).  Every case therefore computes e32, the error of the fp32 torch statement
against its float64 self, and holds the kernel to max(4 * e32, 1e-5 * max|ref|) - 4 for another, equally valid fp32 summation order,
the floor for cases where e32 happens to be tiny - and, unconditionally, to the project's gate of 1e-3 * max|ref|.
With SSR_SSIM_LOSS_REPORT=<file> the observed figures are appended to that file (kept as profiles/ssim_loss/observed_errors.txt)."""
import json
import os

import pytest
import torch

from conftest import GOLDEN
from test_gpu_support_kernels import EINVAL, EUNSUP, Guarded, ibits, same_bits

pytestmark = pytest.mark.gpu

TILE = 32                        # csrc/ssim.hip: one workgroup per (image, 32 x 32 tile)
U = 2.0 ** -24
_REPORT = []


def note(line):
    _REPORT.append(line)
    print(line)


@pytest.fixture(scope="module", autouse=True)
def _report_file(request):
    yield
    path = os.environ.get("SSR_SSIM_LOSS_REPORT")
    if path and _REPORT:
        with open(path, "a") as f:
            f.write(f"# {request.module.__name__}\n" + "\n".join(_REPORT) + "\n")
        del _REPORT[:]


def _hip():
    from satlas_super_resolution_amd import hip
    return hip, hip.lib()


def _family(name, n, c, h, w, seed):
    """NCHW float64 in [0, 1]: uniform noise; a smooth ramp plus 0.02 noise; a mixed image - noise with a band where x == y exactly,
    a flat region at 1.0 in both and a flat 0 against 1 region"""
    g = torch.Generator().manual_seed(seed)
    x, y = torch.rand(n, c, h, w, generator=g, dtype=torch.float64), torch.rand(n, c, h, w, generator=g, dtype=torch.float64)
    if name == "ramp":
        ramp = (torch.arange(h, dtype=torch.float64)[:, None] / h + torch.arange(w, dtype=torch.float64)[None, :] / w) * 0.45 + 0.03
        x, y = ramp + 0.02 * x, ramp + 0.02 * y
    elif name == "mixed":
        a, b = (h + 2) // 3, (2 * h + 2) // 3
        y[..., :a, :] = x[..., :a, :]
        x[..., a:b, :w // 2] = 1.0
        y[..., a:b, :w // 2] = 1.0
        x[..., a:b, w // 2:] = 0.0
        y[..., a:b, w // 2:] = 1.0
    else:
        assert name == "noise"
    return x, y


FAMILIES = ("noise", "ramp", "mixed")


def _reference(x, y, weight):
    """float64 loss and gradient, and the fp32 statement's own error against them: (l64, g64, e32_loss, e32_grad)"""
    from satlas_super_resolution_amd import ssim_loss as SL
    l64, g64 = SL.ssim_loss_grad_reference(x, y, weight)
    xa = x.float().requires_grad_(True)
    l32 = SL.ssim_loss_reference(xa, y.float(), weight)
    l32.backward()
    return float(l64), g64, abs(float(l32.detach()) - float(l64)), float((xa.grad.double() - g64).abs().max())


def _bounds(l64, g64, e32_l, e32_g):
    gmax = float(g64.abs().max())
    bl, bg = max(4 * e32_l, 1e-5 * abs(l64)), max(4 * e32_g, 1e-5 * gmax)
    assert bl <= 1e-3 * abs(l64) and bg <= 1e-3 * gmax, "the inputs keep the derived bound under the project's gate"
    return bl, bg


def _nhwc(t, cs, coff, tdt, fill=None):
    """NCHW values -> channels [coff, coff + C) of a guarded [N, H, W, cs] buffer of `tdt` whose other channels (and, with fill=False,
    the valid ones too) hold the NaN sentinel: (Guarded, ssr_view)"""
    hip, _ = _hip()
    n, c, h, w = t.shape
    g = Guarded(n * h * w * cs, tdt)
    v = g.t.view(n, h, w, cs)
    if fill is not False:
        v[..., coff:coff + c] = t.permute(0, 2, 3, 1).to(tdt).cuda()
    return g, hip.View(g.ptr(), cs, coff)


def _read(g, shape, cs, coff):
    n, c, h, w = shape
    return g.t.view(n, h, w, cs)[..., coff:coff + c].double().cpu().permute(0, 3, 1, 2)


def _launch(vx, vy, vg, code, shape, weight, acc, loss_ptr):
    hip, L = _hip()
    n, c, h, w = shape
    return L.ssr_ssim_loss(vx, vy, vg, code, n, h, w, c, weight, acc, loss_ptr, hip.stream_ptr())


def _check_case(tag, x, y, mode, weight=0.1, lay=((8, 0), (8, 0), (8, 0))):
    """one (inputs, storage type, layout): the null-gradient form, accumulate 0 and accumulate 1"""
    hip, _ = _hip()
    code = hip.dtype_code(mode)
    tdt = hip.torch_dtype(code)
    x, y = x.to(tdt).double(), y.to(tdt).double()          # the float64 reference takes the storage-rounded inputs
    shape = tuple(x.shape)
    l64, g64, e32_l, e32_g = _reference(x, y, weight)
    bl, bg = _bounds(l64, g64, e32_l, e32_g)
    gmax = float(g64.abs().max())
    (xcs, xco), (ycs, yco), (gcs, gco) = lay
    gx, vx = _nhwc(x, xcs, xco, tdt)
    gy, vy = _nhwc(y, ycs, yco, tdt)
    old = (0.5 * gmax * torch.randn(shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)).to(tdt).double()
    for form in ("null", "write", "add"):
        gl = Guarded(1)
        gl.t.zero_()
        if form == "null":
            gg, vg = None, hip.NULL_VIEW
        else:
            gg, vg = _nhwc(old, gcs, gco, tdt, fill=(form == "add"))      # "write": the valid channels start as NaN too
        assert _launch(vx, vy, vg, code, shape, weight, int(form == "add"), gl.ptr()) == 0
        torch.cuda.synchronize()
        el = abs(float(gl.t[0]) - l64)
        note(f"{tag:<34} {mode:<5} {form:<5} loss err {el:.3e} bound {bl:.3e} (e32 {e32_l:.3e})")
        assert el <= bl, (tag, mode, form, el, bl)
        assert gl.margins_intact() and gx.margins_intact() and gy.margins_intact()
        if gg is None:
            continue
        got = _read(gg, shape, gcs, gco)
        assert bool(torch.isfinite(got).all()), (tag, mode, form)
        ref = g64 + old if form == "add" else g64
        err = (got - ref).abs()
        if mode == "bf16":
            from oracle.layerwise import bf16_ulp
            # within one bf16 ulp of rnd(old + g64), plus the fp32 bound as slack
            rr = ref.float().bfloat16().double()
            ok = (got - rr).abs() <= bf16_ulp(rr.abs().float()).double() * 1.0001 + bg
            note(f"{tag:<34} {mode:<5} {form:<5} grad err/ulp-bound max {float(((got - rr).abs() / (bf16_ulp(rr.abs().float()).double() + bg)).max()):.3f}")
            assert bool(ok.all()), (tag, mode, form, float(err.max()), gmax)
        else:
            # the fp32 bound, plus for "add" the one rounding of the stored sum
            bound = bg + (U * ref.abs() if form == "add" else 0.0)
            note(f"{tag:<34} {mode:<5} {form:<5} grad err {float(err.max()):.3e} = {float(err.max()) / gmax:.2e} max|g|  bound {bg:.3e} "
                 f"(e32 {e32_g:.3e}; err / e32 {float(err.max()) / max(e32_g, 1e-300):.2f})")
            assert bool((err <= bound).all()), (tag, mode, form, float(err.max()), bg, gmax)
        assert gg.margins_intact() and gg.channels_intact(gcs, gco, shape[1]), "padding channels / guard bands of grad"
        assert gx.channels_intact(xcs, xco, shape[1]) and gy.channels_intact(ycs, yco, shape[1])


# folds from one and from both ends; one below / at / one above the tile edge in each dimension; two tiles plus a remainder; a size
# with no relation to the tile; the training shape of one image
SHAPES = [(2, 3, 3), (1, 3, 4), (2, 4, 5), (2, 5, 7), (1, 31, 33), (1, 32, 32), (1, 33, 31), (1, 65, 70), (2, 37, 53), (1, 128, 128)]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("n,h,w", SHAPES, ids=[f"{n}x{h}x{w}" for n, h, w in SHAPES])
def test_kernel_matches_float64(n, h, w, mode):
    for fam in FAMILIES:
        x, y = _family(fam, n, 3, h, w, seed=h * 1000 + w)
        _check_case(f"{n}x3x{h}x{w} {fam}", x, y, mode)


# C = 1; three channels at a non-zero offset of wider buffers (all three layouts different); seven channels = two full channel
# groups of the kernel and a remainder
LAYOUTS = [(1, ((8, 0), (8, 0), (8, 0))), (3, ((16, 5), (24, 16), (16, 8))), (7, ((8, 0), (8, 1), (8, 0)))]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("c,lay", LAYOUTS, ids=["C1", "C3-offset", "C7"])
def test_kernel_channel_counts_and_offsets(c, lay, mode):
    for fam in ("noise", "mixed"):
        x, y = _family(fam, 2, c, 37, 53, seed=c)
        _check_case(f"2x{c}x37x53 {fam} {lay[0]}", x, y, mode, lay=lay)


def test_fp32x3_storage_code_is_fp32():
    hip, _ = _hip()
    x, y = _family("noise", 1, 3, 9, 6, seed=3)
    g1, v1 = _nhwc(x.float(), 8, 0, torch.float32)
    g2, v2 = _nhwc(y.float(), 8, 0, torch.float32)
    outs = []
    for code in (hip.F32, hip.F32X3):
        gg, vg = _nhwc(x, 8, 0, torch.float32, fill=False)
        gl = Guarded(1)
        gl.t.zero_()
        assert _launch(v1, v2, vg, code, (1, 3, 9, 6), 0.1, 0, gl.ptr()) == 0
        outs.append((gg, gl))
    torch.cuda.synchronize()
    assert same_bits(outs[0][0].buf, outs[1][0].buf) and same_bits(outs[0][1].buf, outs[1][1].buf)


@pytest.mark.parametrize("n,h,w", [(3, 70, 45), (29, 65, 70)], ids=["18-tiles", "261-tiles"])
def test_determinism_and_loss_slots(n, h, w):
    """the gradient is a gather: same bytes from two launches with and without SSR_DETERMINISTIC; under the flag block b is the single
    writer of slot b, the grid is min(tiles, SSR_LOSS_SLOTS) (261 tiles: some blocks walk two) and the slots added in index order
    meet the loss bound"""
    hip, _ = _hip()
    shape = (n, 3, h, w)
    x, y = _family("noise", n, 3, h, w, seed=11)
    x, y = x.float().double(), y.float().double()
    l64, g64, e32_l, e32_g = _reference(x, y, 0.1)
    bl, _ = _bounds(l64, g64, e32_l, e32_g)
    gx, vx = _nhwc(x, 8, 0, torch.float32)
    gy, vy = _nhwc(y, 8, 0, torch.float32)
    tiles = n * ((h + TILE - 1) // TILE) * ((w + TILE - 1) // TILE)
    grid = min(tiles, hip.LOSS_SLOTS)
    grads, slots = [], []
    for flag in (0, 0, hip.DETERMINISTIC, hip.DETERMINISTIC):
        gg, vg = _nhwc(x, 8, 0, torch.float32, fill=False)
        gl = Guarded(hip.LOSS_SLOTS if flag else 1)
        gl.t[:grid if flag else 1] = 0.0
        assert _launch(vx, vy, vg, hip.F32 | flag, shape, 0.1, 0, gl.ptr()) == 0
        torch.cuda.synchronize()
        grads.append(gg)
        slots.append(gl)
        assert gl.margins_intact() and gg.margins_intact()
    for g in grads[1:]:
        assert same_bits(grads[0].buf, g.buf)
    assert same_bits(slots[2].buf, slots[3].buf)
    det = slots[2]
    assert bool((ibits(det.t)[grid:] == det.sent).all()), "slots at and beyond the grid are untouched"
    total = 0.0
    for v in det.t[:grid].double().cpu().tolist():      # index order
        total += v
    el = abs(total - l64)
    note(f"{n}x3x{h}x{w} det slots ({grid} of {tiles} tiles) loss err {el:.3e} bound {bl:.3e}")
    assert el <= bl
    assert abs(float(slots[0].t[0]) - l64) <= bl
    # `+=`: a second launch into the same slots doubles them (one writer per slot, launches on a stream are ordered)
    first = det.t[:grid].clone()
    assert _launch(vx, vy, hip.NULL_VIEW, hip.F32 | hip.DETERMINISTIC, shape, 0.1, 0, det.ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(det.t[:grid], first + first)


def test_refusals_leave_outputs_untouched():
    hip, _ = _hip()
    x, y = _family("noise", 1, 3, 4, 4, seed=1)
    gx, vx = _nhwc(x, 8, 0, torch.float32)
    gy, vy = _nhwc(y, 8, 0, torch.float32)
    gg, vg = _nhwc(x, 8, 0, torch.float32, fill=False)
    gl = Guarded(1)

    def call(vx_=vx, code=hip.F32, n=1, h=4, w=4, c=3):
        return _hip()[1].ssr_ssim_loss(vx_, vy, vg, code, n, h, w, c, 0.1, 0, gl.ptr(), hip.stream_ptr())
    assert call(h=2) == EINVAL and call(w=2) == EINVAL and call(c=0) == EINVAL and call(n=0) == EINVAL
    assert call(vx_=hip.View(None, 8, 0)) == EINVAL
    assert call(c=9) == EINVAL                                       # wider than the view
    assert call(code=7) == EUNSUP and call(code=hip.F32H3) == EUNSUP
    torch.cuda.synchronize()
    for g in (gg, gl):
        assert bool((ibits(g.buf) == g.sent).all())


# ------------------------------------------------------------------------------------------------ the term inside the train step
SSIM_W = 0.1      # the shipped block's loss_weight (ssimloss_esrgan_s2naip_urban.yml)
# the oracle test's weight: at the shipped 0.1 the term moves the tiny generator's gradients by 8.7e-3 of their maximum (CPU, both
# oracles), under ten times the 2e-3 gate; the movement is linear in the weight, 1.0 gives 8e-2
STEP_W = 1.0


def _with_ssim(monkeypatch, w):
    """oracle.esrgan_oracle.perceptual_loss + the SSIM term, patched in for the duration of a test: the reference passes the same two
    tensors (self.output, percep_gt) to both losses (ssr_esrgan_model.py:153-166)"""
    from oracle import esrgan_oracle as O
    from satlas_super_resolution_amd.ssim_loss import ssim_loss_reference
    orig = O.perceptual_loss

    def wrapped(vgg_sd, x, gt, layer_weights, perceptual_weight=1.0, use_input_norm=True, range_norm=False, prec=O.FP32):
        return orig(vgg_sd, x, gt, layer_weights, perceptual_weight, use_input_norm, range_norm, prec) + ssim_loss_reference(x, gt.detach(), w)
    monkeypatch.setattr(O, "perceptual_loss", wrapped)


def _tiny_step_setup(perceptual=True, weight=None):
    from oracle import esrgan_oracle as O
    from satlas_super_resolution_amd.models.ssr_esrgan_model import train_config_from_opt
    opt = json.load(open(os.path.join(GOLDEN, "ssr_options.json")))["ssimloss_esrgan_s2naip_urban.yml"]
    opt["feed_disc_lr"] = False
    if not perceptual:
        del opt["train"]["perceptual_opt"]
    if weight is not None:
        opt["train"]["ssim_opt"]["loss_weight"] = weight
    cfg = train_config_from_opt(opt)
    g_kw = dict(num_in_ch=6, num_out_ch=3, scale=4, num_feat=16, num_block=1, num_grow_ch=8)
    d_kw = dict(num_in_ch=3, num_feat=8, skip_connection=True)
    g0, d0 = O.generator_init(seed=41, **g_kw), O.discriminator_init(3, 8, seed=42)
    vgg = O.vgg19_init(seed=43)
    torch.manual_seed(44)
    lr, gt = torch.rand(2, 6, 16, 16), torch.rand(2, 3, 64, 64)
    return cfg, g_kw, d_kw, g0, d0, vgg, lr, gt


def test_train_step_with_shipped_ssimloss_block_matches_oracle(monkeypatch):
    from oracle import esrgan_oracle as O
    from satlas_super_resolution_amd.train_step import ESRGANTrainStep
    cfg, g_kw, d_kw, g0, d0, vgg, lr, gt = _tiny_step_setup(weight=STEP_W)
    assert cfg.ssim == {"loss_weight": STEP_W} and cfg.perceptual and cfg.percep_gt_usm
    ocfg = lambda c: O.StepConfig(l1_weight=c.l1_weight, gan_weight=c.gan_weight, lr_g=c.lr_g, lr_d=c.lr_d, betas=c.betas,
                                  ema_decay=c.ema_decay, l1_gt_usm=True, gan_gt_usm=False, percep_gt_usm=True, perceptual=c.perceptual)
    plain = O.ESRGANOracle(g0, d0, ocfg(cfg), vgg_sd=vgg)
    plain.step(lr, gt, 1)
    _with_ssim(monkeypatch, STEP_W)
    orc = O.ESRGANOracle(g0, d0, ocfg(cfg), vgg_sd=vgg)
    ref_log = orc.step(lr, gt, 1)
    # the term matters: some generator gradient moves by more than ten times the gate below
    moved = max(float((orc.g_grads[k] - plain.g_grads[k]).abs().max() / orc.g_grads[k].abs().max()) for k in orc.g_grads)
    assert moved > 10 * 2e-3, moved
    ts = ESRGANTrainStep(g_kw, d_kw, 2, 16, 16, "fp32", cfg, use_graph=False, vgg_state=vgg)
    ts.load_state(g0, d0)
    ts.feed_data(lr.cuda(), gt.cuda())
    ts.step(1)
    log = ts.log()
    assert set(log) == set(ref_log) | {"l_g_ssim"} and log["l_g_ssim"] > 0
    for k, v in ref_log.items():
        got = log[k] + log["l_g_ssim"] if k == "l_g_percep" else log[k]
        assert abs(got - v) <= 1e-3 * max(1.0, abs(v)), (k, got, v)
    for k, g in orc.g_grads.items():                       # the bounds of tests/test_gpu_style_loss.py
        got = ts.g_store.tensor(k, ts.g_store.grad)
        gc_, gr_ = got.detach().float().cpu(), g.detach().float().cpu()
        err, scale = (gc_ - gr_).abs(), float(gr_.abs().max())
        outside = int((err > 2e-3 * (scale + gr_.abs())).sum())
        assert outside <= max(3, int(2e-3 * err.numel())) and float(err.max()) <= 1e-2 * scale and float(err.mean()) <= 1e-3 * scale, \
            (k, outside, err.numel(), float(err.max()) / scale)
    ts2 = ESRGANTrainStep(g_kw, d_kw, 2, 16, 16, "fp32", cfg, use_graph=True, vgg_state=vgg)     # hipGraph replay of the same step
    ts2.load_state(g0, d0)
    ts2.feed_data(lr.cuda(), gt.cuda())
    for it in (1, 2, 3):
        ts2.step(it)
    log2 = ts2.log()
    assert "l_g_ssim" in log2 and all(v == v and abs(v) != float("inf") for v in log2.values())


def test_ssim_without_perceptual_opt_uses_the_sharpened_target():
    """no perceptual_opt, percep_gt_usm set, fp32h: the term still takes the USM-sharpened ground truth; l_g_ssim and the image
    gradient against the CPU statement on the device's own output"""
    from oracle import esrgan_oracle as O
    from satlas_super_resolution_amd import ssim_loss as SL
    from satlas_super_resolution_amd.train_step import ESRGANTrainStep
    cfg, g_kw, d_kw, g0, d0, vgg, lr, gt = _tiny_step_setup(perceptual=False)
    assert cfg.perceptual is None and cfg.percep_gt_usm and cfg.l1_gt_usm and cfg.ssim
    ts = ESRGANTrainStep(g_kw, d_kw, 2, 16, 16, "fp32h", cfg, use_graph=False)
    assert ts.p_plan is None and ts.percep_tgt is not None
    ts.load_state(g0, d0)
    ts.feed_data(lr.cuda(), gt.cuda())
    ts.step(1)
    log = ts.log()
    assert set(log) == {"l_g_pix", "l_g_gan", "l_g_ssim", "l_d_real", "out_d_real", "l_d_fake", "out_d_fake"}
    out = ts.output().double().cpu()
    # the oracle's USMSharp applied in float64, as tests/test_gpu_metric_kernels.py holds ssr_usm_sharp to it: evaluated in fp32 its
    # threshold mask differs from its own float64 evaluation at a pixel of this image (4e-4 in the target, 3e-4 of max|grad|)
    tgt = O.usm_sharp(gt.double())
    l64, g64, e32_l, e32_g = _reference(out, tgt, SSIM_W)
    bl, bg = _bounds(l64, g64, e32_l, e32_g)
    note(f"step, no perceptual_opt: l_g_ssim err {abs(log['l_g_ssim'] - l64):.3e} bound {bl:.3e}")
    assert abs(log["l_g_ssim"] - l64) <= bl
    assert abs(log["l_g_ssim"] - float(SL.ssim_loss_reference(out, tgt, SSIM_W))) <= bl
    # grad_l1 = the L1 gradient (exact: +-weight / numel from the device's own buffers) + the SSIM gradient
    fake, l1t = ts.fake_in[..., :3].double().cpu(), ts.l1_tgt[..., :3].double().cpu()
    l1g = (cfg.l1_weight / out.numel()) * torch.sign(fake - l1t).permute(0, 3, 1, 2)
    got = ts.grad_l1[..., :3].double().cpu().permute(0, 3, 1, 2)
    ref = l1g.float().double() + g64
    err = (got - ref).abs()
    note(f"step, no perceptual_opt: grad_l1 err {float(err.max()):.3e} bound {bg:.3e} (max|g_ssim| {float(g64.abs().max()):.3e})")
    assert bool((err <= bg + 2 * U * ref.abs()).all()), (float(err.max()), bg)      # + the rounding of the L1 constant and of the sum
    assert float(ts.grad_l1[..., 3:].abs().max()) == 0.0


def test_ssim_term_is_deterministic_in_fp32h():
    from satlas_super_resolution_amd.train_step import ESRGANTrainStep
    cfg, g_kw, d_kw, g0, d0, vgg, lr, gt = _tiny_step_setup()
    cfg.deterministic = True
    B = 4
    lr, gt = lr.repeat(2, 1, 1, 1), gt.repeat(2, 1, 1, 1)
    runs = []
    for _ in range(2):
        ts = ESRGANTrainStep(g_kw, d_kw, B, 16, 16, "fp32h", cfg, use_graph=True, vgg_state=vgg)
        ts.load_state(g0, d0)
        ts.feed_data(lr.cuda(), gt.cuda())
        for it in (1, 2):
            ts.step(it)
        log = ts.log()
        runs.append((log["l_g_ssim"], ts.output().cpu(), ts.g_store.data.detach().cpu().clone()))
    assert runs[0][0] == runs[1][0] and runs[0][0] > 0
    assert torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2], runs[1][2])


def test_model_plugin_runs_the_shipped_ssimloss_option(tmp_path, monkeypatch):
    from satlas_super_resolution_amd import models, perceptual as P  # noqa: F401
    from satlas_super_resolution_amd.registry import build_model
    opt = json.load(open(os.path.join(GOLDEN, "ssr_options.json")))["ssimloss_esrgan_s2naip_urban.yml"]
    opt.update(is_train=True, dist=False, rank=0, world_size=1, compute_dtype="fp32h")
    opt["path"].update(models=str(tmp_path / "models"), training_states=str(tmp_path / "states"), visualization=str(tmp_path / "vis"))
    opt["network_d"]["num_in_ch"] = 3 + opt["network_g"]["num_in_ch"]     # as in test_gpu_boundary: the shipped D width cannot run
    opt["network_g"]["num_block"] = 2                                     # the loss plumbing is under test, not the body's depth
    wfile = tmp_path / "vgg19-dcbb9e9d.pth"
    torch.save(P.vgg19_random_state(P.vgg19_specs("conv5_4"), seed=1), wfile)
    monkeypatch.setenv("SSR_VGG19_WEIGHTS", str(wfile))
    model = build_model(json.loads(json.dumps(opt)))
    assert model.cfg.ssim == {"loss_weight": SSIM_W}
    g = torch.Generator().manual_seed(0)
    for it in (1, 2):
        model.update_learning_rate(it, warmup_iter=-1)
        model.feed_data({"lr": torch.randint(0, 256, (2, 36, 32, 32), generator=g, dtype=torch.uint8),
                         "hr": torch.randint(0, 256, (2, 3, 128, 128), generator=g, dtype=torch.uint8)})
        model.optimize_parameters(it)
    log = model.get_current_log()
    assert set(log) == {"l_g_pix", "l_g_percep", "l_g_ssim", "l_g_gan", "l_d_real", "out_d_real", "l_d_fake", "out_d_fake"}
    assert 0 < log["l_g_ssim"] < float("inf")
    bad = json.loads(json.dumps(opt))
    bad["train"]["ssim_opt"]["type"] = "Other"
    with pytest.raises(NotImplementedError, match="ssim_opt"):
        build_model(bad)
