"""The finish of the register-tiled body kernel (csrc/conv_x3r.hip): every MFMA wave stores its K-quarter partial tiles in pixel-row
layout, then all threads of the workgroup sum the quarters of their items (one pixel x four channels), apply the straight-line
epilogue (bias + LeakyReLU; alpha, bias, r1, r2; mask) on operands requested before the barriers and store 16 bytes.

Checked per case: agreement with a float64 torch reference inside the bound tests/test_gpu_conv_x3.py holds each arithmetic mode to;
the same bytes from the half-height (TH = 4) and the full-height (TH = 8) tiling of the same images - the launch shape picks the tiling,
as in tests/test_gpu_conv_x3.py, so the images are computed in a small and in a large batch - and, at 64 output channels, from the form
with two channel tiles per wave; the same bytes from two runs; and a sentinel in every channel and pixel of the strided destination
that the layer does not own."""
import ctypes as C
import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu

# the bounds of tests/test_gpu_conv_x3.py (TOL: split-bf16; its 2e-6: exact fp32; H_TOL: fp16-split), of max|ref|
TOLS = {"fp32x3": 1e-4, "fp32": 2e-6, "fp32h": 2e-6}
AM = {"fp32x3": 0, "fp32": 1, "fp32h": 2}
SENTINEL = -777.0
GRIDS = [(8, 16), (12, 20), (32, 32)]                 # one tile; partial tiles on both axes; 4 x 2 full-height tiles
CINS = ["16", "48", "32+32"]                          # one chunk (an MFMA wave without work); three; two views of two chunks each
FORMS = ["lrelu", "lin_r1_r2", "lin_r1", "lin", "mask"]
EP = {"lrelu": 0, "lin_r1_r2": 1, "lin_r1": 1, "lin": 1, "mask": 2}


def _mods():
    from satlas_super_resolution_amd import engine, hip
    return engine, hip


def _cin(spec):
    return sum(int(c) for c in spec.split("+"))


@functools.lru_cache(maxsize=None)
def _data(H, W, spec, cout):
    """two images, weights, epilogue operands and the float64 convolution of one (grid, input, output) shape: made once, never changed"""
    g = torch.Generator().manual_seed(10 * _cin(spec) + cout + len(spec))
    cin = _cin(spec)
    rn = lambda *s: torch.randn(*s, generator=g)
    w = rn(cout, cin, 3, 3) * (1.0 / (cin * 9) ** 0.5)         # (drawn first: the same weights on every grid)
    b = rn(cout) * 0.1
    x = rn(2, H, W, cin) * 0.5
    r1, r2, m = rn(2, H, W, cout) * 0.5, rn(2, H, W, cout) * 0.5, rn(2, H, W, cout) * 0.5
    acc = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    return dict(x=x, w=w, b=b, r1=r1, r2=r2, m=m, acc=acc)


def _reference(dat, form):
    acc = dat["acc"]
    if form == "lrelu":
        return F.leaky_relu(acc, 0.2)
    if form == "mask":
        return acc * torch.where(dat["m"] > 0, torch.tensor(1.0, dtype=torch.float64), torch.tensor(0.2, dtype=torch.float64))
    ref = 0.04 * acc
    if form in ("lin_r1", "lin_r1_r2"):
        ref = ref + 0.2 * dat["r1"].double()
    if form == "lin_r1_r2":
        ref = ref + 1.0 * dat["r2"].double()
    return ref


@functools.lru_cache(maxsize=None)
def _store(spec, cout, mode):
    engine, hip = _mods()
    dat = _data(GRIDS[0][0], GRIDS[0][1], spec, cout)
    st = engine.ParamStore([engine.ConvSpec("c", cout, _cin(spec), 3, 1, True, False)], hip.dtype_code(mode))
    st.load_state_dict({"c.weight": dat["w"], "c.bias": dat["b"]})
    st.pack()
    return st


def _launch(H, W, spec, cout, mode, form, N):
    """the two images of _data repeated to a batch of N -> (the whole destination buffer, the symbol of the kernel launched)"""
    engine, hip = _mods()
    dat = _data(H, W, spec, cout)
    st = _store(spec, cout, mode)
    Ho, Wo, YC, YOFF = H + 1, W + 2, cout + 24, 8               # a destination wider, taller and deeper than the layer's output
    rep = lambda t: t.repeat(N // 2, 1, 1, 1)

    def widen(t, c_total, coff, h=H, w=W):                      # [N, h, w, c_total] on the device with t at channel coff
        buf = torch.randn(N, h, w, c_total) * 0.5
        buf[:, :H, :W, coff:coff + t.shape[-1]] = rep(t)
        return buf.cuda().contiguous()

    parts = [int(c) for c in spec.split("+")]
    xs, c0 = [], 0
    for c in parts:
        xs.append((widen(dat["x"][..., c0:c0 + c], c + 32, 16), c))
        c0 += c
    r1, r2, m = (widen(dat[k], cout + 8, 4, Ho, Wo) for k in ("r1", "r2", "m"))
    y = torch.full((N, Ho, Wo, YC), SENTINEL, device="cuda")
    kw = dict(act=hip.ACT_LRELU if form == "lrelu" else hip.ACT_NONE, cin=parts[0])
    if form.startswith("lin"):
        kw.update(alpha=0.04)
    if form in ("lin_r1", "lin_r1_r2"):
        kw.update(r1=hip.view(r1, 4), r1_nc=cout, beta1=0.2)
    if form == "lin_r1_r2":
        kw.update(r2=hip.view(r2, 4), r2_nc=cout, beta2=1.0)
    cb = engine._ConvBuilder(st, N)
    d = cb.conv(engine.Launcher(), "c", hip.view(xs[0][0], 16), H, W, hip.view(y, YOFF), **kw)
    d.Ho, d.Wo = Ho, Wo
    if len(xs) == 2:
        d.x2, d.Cin2 = hip.view(xs[1][0], 16), xs[1][1]
    if form == "mask":
        d.m, d.m_c0, d.m_c1 = hip.view(m, 4), 0, cout
    hip.check(hip.lib().ssr_conv2d_impl(C.byref(d), hip.stream_ptr(), 7), "impl 7")
    torch.cuda.synchronize()
    return y, hip.conv_symbol(d)


def _owned(y, H, W, cout):
    return y[:, :H, :W, 8:8 + cout]


def _batch_for(H, W, cout, wide):
    """the smallest even batch whose launch takes full-height tiles (conv_x3r.hip, xr_tile_height: more than 160 workgroups of 8 x 16
    pixels x 32 channels); wide: ... and whose 64-channel layer runs as one workgroup per tile (xr_wide_form: more than 160 tiles)"""
    per = ((W + 15) // 16) * ((H + 7) // 8)
    need = 160 if wide else 160 // (cout // 32)
    n = need // per + 1
    return n + (n & 1)


def _check_case(H, W, spec, cout, mode, form, symbols):
    """symbols: {name: (batch, expected instantiation)}; the first is the small launch everything else is compared with"""
    dat = _data(H, W, spec, cout)
    names = list(symbols)
    outs = {}
    for nm in names:
        y, sym = _launch(H, W, spec, cout, mode, form, symbols[nm][0])
        assert sym == symbols[nm][1], (nm, sym, symbols[nm][1])
        outs[nm] = y
    y = outs[names[0]]
    e = rel_err(_owned(y, H, W, cout).cpu().double(), _reference(dat, form))
    print(f"[{mode} {form} {H}x{W} cin {spec} cout {cout}] {e:.2e} of max|ref| (bound {TOLS[mode]:g})")
    assert e < TOLS[mode], e
    # what the layer does not own: the other channels of the destination, the rows and columns beyond the grid
    keep = torch.ones_like(y, dtype=torch.bool)
    keep[:, :H, :W, 8:8 + cout] = False
    assert bool((y[keep] == SENTINEL).all())
    assert bool((_owned(y, H, W, cout) != SENTINEL).all())
    # two runs: the same bytes
    y_again, _ = _launch(H, W, spec, cout, mode, form, symbols[names[0]][0])
    assert torch.equal(y.view(torch.int32), y_again.view(torch.int32))
    # the other tilings / forms: the same bytes per image, and nothing else touched
    for nm in names[1:]:
        yb = outs[nm]
        assert torch.equal(yb[:2].view(torch.int32), y.view(torch.int32)), (nm, symbols[nm][1])
        assert torch.equal(yb[-2:].view(torch.int32), y.view(torch.int32)), (nm, symbols[nm][1], "last images")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", ["fp32x3", "fp32h", "fp32"])
@pytest.mark.parametrize("cout", [32, 64])
@pytest.mark.parametrize("spec", CINS)
@pytest.mark.parametrize("H,W", GRIDS)
def test_finish_by_items(H, W, spec, cout, mode, form):
    ep, am = EP[form], AM[mode]
    symbols = {"half height": (2, f"conv_x3r_kernel<1, 1, {ep}, 4, {am}>"),
               "full height": (_batch_for(H, W, cout, False), f"conv_x3r_kernel<1, 1, {ep}, 8, {am}>")}
    if cout == 64 and (H, W) != (32, 32):
        symbols["two channel tiles per wave"] = (_batch_for(H, W, cout, True), f"conv_x3r_kernel<2, 1, {ep}, 8, {am}>")
    _check_case(H, W, spec, cout, mode, form, symbols)


def _twelve_wave_main():
    """(child process of the test below: SSR_X3_REGTILE_NT2=8 is read once per process)"""
    for H, W in GRIDS[:2]:
        for spec in ("16", "32+32"):
            for form in FORMS:
                ep = EP[form]
                _check_case(H, W, spec, 64, "fp32x3", form,
                            {"half height": (2, f"conv_x3r_kernel<1, 1, {ep}, 4, 0>"),
                             "twelve waves": (_batch_for(H, W, 64, True), f"conv_x3r_kernel<1, 2, {ep}, 8, 0>")})
    print("twelve-wave form ok")


def test_finish_by_items_twelve_wave_form():
    """the 64-channel layers on eight MFMA waves (SSR_X3_REGTILE_NT2=8): 2048 items over 768 threads, a last round short by four waves"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, SSR_X3_REGTILE_NT2="8")
    code = f"import sys; sys.path.insert(0, {here!r}); import test_gpu_conv_x3r_finish as t; t._twelve_wave_main()"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "twelve-wave form ok" in r.stdout
