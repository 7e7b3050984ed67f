"""GPU: the CLIPScore metric (`calculate_clipscore`): the C-ABI entries of csrc/vit.hip on their own (ssr_linear against float64
F.linear within a derived bound, ssr_layernorm_fwd, ssr_mha_fwd, ssr_vit_patch_input bit-exact, ssr_vit_tokens, ssr_cosine_pairs),
the whole tower against clip_image_features_reference in float64, and the metric through the model plugin's test pipeline.  Inputs
and outputs are channel slices of wider NaN-filled buffers: nothing outside a view is read or written.  The figures these tests
printed on an MI355X are in profiles/clipscore/observed_errors.txt."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clipscore_fixture as FX
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24          # unit roundoff of fp32


def _padded(x2d, cs, coff, device="cuda"):
    """x [rows, c] -> a NaN buffer [rows, cs] holding x at channel coff, on the device"""
    b = torch.full((x2d.shape[0], cs), float("nan"))
    b[:, coff:coff + x2d.shape[1]] = x2d
    return b.to(device)


def _V(t, coff=0):
    from satlas_super_resolution_amd import hip
    return hip.View(t.data_ptr(), t.shape[-1], coff)


# ------------------------------------------------------------------ ssr_linear
# the issue's seven shapes run the 64 x 64 tile (fewer than 256 tiles of 128 x 128); the last, SO400M's packed qkv at a batch of two, has
# 12 x 27 = 324 and runs the 128 x 128 tile, so its rows-subset check compares the two tile shapes bit for bit
LINEAR_CASES = [(10, 144, 432), (1, 144, 200), (33, 200, 144), (394, 768, 3072), (197, 3072, 768), (729, 1152, 4304), (729, 4304, 1152),
                (1458, 1152, 3456)]
# (bias, activation, residual: None | 'view' | 'in place')
LINEAR_VARIANTS = {"plain": (False, "none", None), "bias": (True, "none", None), "bias+res in place": (True, "none", "in place"),
                   "res": (False, "none", "view"), "bias+quick_gelu": (True, "quick_gelu", None), "bias+gelu_tanh+res": (True, "gelu_tanh", "view"),
                   "bias+gelu_erf": (True, "gelu_erf", None), "gelu_tanh": (False, "gelu_tanh", None)}
ACTS = {"none": lambda v: v, "quick_gelu": lambda v: v * torch.sigmoid(1.702 * v), "gelu_tanh": lambda v: F.gelu(v, approximate="tanh"),
        "gelu_erf": lambda v: F.gelu(v)}
# the largest slope of each activation (quick_gelu: 1.0998 at x = 1.06; both GELUs: 1.129 at x = 1.41), rounded up
LIPSCHITZ = {"none": 1.0, "quick_gelu": 1.1, "gelu_tanh": 1.13, "gelu_erf": 1.13}


@functools.lru_cache(maxsize=None)
def _linear_case(M, K, Nout):
    """inputs and the float64 products of one shape, computed once for all its variants"""
    g = torch.Generator().manual_seed(M * 7919 + K * 31 + Nout)
    x, w = torch.randn(M, K, generator=g), torch.randn(Nout, K, generator=g) / K ** 0.5
    b, r = torch.randn(Nout, generator=g), torch.randn(M, Nout, generator=g)
    return x, w, b, r, x.double() @ w.double().t(), x.double().abs() @ w.double().abs().t()


def _linear(x, w, b, r, M, K, Nout, act, in_place, rows=None):
    """-> the whole output buffer [rows, Nout + 16] (NaN outside the slice at channel 8) as numpy"""
    from satlas_super_resolution_amd import hip
    rows = rows or M
    xb, wd = _padded(x[:rows], K + 8, 4), w.cuda()
    bd = b.cuda() if b is not None else None
    y = torch.full((rows, Nout + 16), float("nan"), device="cuda")
    rv, keep = hip.NULL_VIEW, None
    if r is not None and in_place:
        y[:, 8:8 + Nout] = r[:rows].cuda()
        rv = _V(y, 8)
    elif r is not None:
        keep = _padded(r[:rows], Nout + 12, 4)
        rv = _V(keep, 4)
    hip.check(hip.lib().ssr_linear(_V(xb, 4), wd.data_ptr(), bd.data_ptr() if bd is not None else None, rv, _V(y, 8), hip.F32, rows, K, Nout,
                                   hip.VIT_ACTS[act], hip.stream_ptr()), "ssr_linear")
    return y.cpu().numpy()


@pytest.mark.parametrize("variant", list(LINEAR_VARIANTS))
@pytest.mark.parametrize("case", LINEAR_CASES, ids=["x".join(map(str, c)) for c in LINEAR_CASES])
def test_linear_matches_float64(case, variant):
    """Bound per output, for ANY fp32 summation order with or without fused multiply-add (the form test_conv_direct_matches_float64
    states), before the activation:
        |err_pre| <= gamma_(K+1) (sum_k |x_k w_k| + |b|) + K 2^-126,   gamma_n = n u / (1 - n u), u = 2^-24
    The activation multiplies it by its Lipschitz constant and adds its own fp32 evaluation error, taken as 4 x the largest deviation
    of torch's fp32 CPU activation from the float64 one on the same pre-activations (a property of evaluating the function in fp32
    over this range, so the maximum over the tensor, not the chance value of one element); the residual addition adds one rounding
    of the result.  Nothing here comes from what the kernel returns."""
    M, K, Nout = case
    has_b, act, res = LINEAR_VARIANTS[variant]
    x, w, b, r, xw, mag = _linear_case(M, K, Nout)
    pre = xw + b.double() if has_b else xw
    want = ACTS[act](pre)
    gamma = (K + 1) * U32 / (1 - (K + 1) * U32)
    tol = LIPSCHITZ[act] * (gamma * (mag + (b.double().abs() if has_b else 0)) + K * 2.0 ** -126)
    act_dev = 0.0
    if act != "none":
        act_dev = float((ACTS[act](pre.float()).double() - want).abs().max())
        tol = tol + 4 * act_dev
    if res:
        want = want + r.double()
        tol = tol + U32 * want.abs()
    want, tol = want.numpy(), (tol.numpy() if torch.is_tensor(tol) else tol)
    args = (x, w, b if has_b else None, r if res else None, M, K, Nout, act, res == "in place")
    y1 = _linear(*args)
    y2 = _linear(*args)
    got = y1[:, 8:8 + Nout]
    assert not np.isnan(got).any()                                           # every output written, nothing outside X[M, K] read
    assert np.isnan(np.delete(y1, np.s_[8:8 + Nout], axis=-1)).all()         # channels outside the output slice untouched
    assert y1.tobytes() == y2.tobytes()                                      # a second launch: the same bytes
    few = min(M, 5)
    assert _linear(*args, rows=few).tobytes() == y1[:few].tobytes()          # fewer rows (the 64 x 64 tile, whatever tile M rows took): the same bytes
    err = np.abs(got.astype(np.float64) - want)
    print(f"ssr_linear {M}x{K}x{Nout} {variant}: max |err| {err.max():.3e}, max err / bound {np.max(err / tol):.3f}, fp32 CPU activation deviation {act_dev:.3e}")
    assert (err <= tol).all(), (float(err.max()), float(np.max(err / tol)))


def test_linear_error_codes():
    from satlas_super_resolution_amd import hip
    L = hip.lib()
    x = torch.zeros(8, 16, device="cuda")
    w = torch.zeros(8, 16, device="cuda")
    y = torch.full((8, 8), 7.0, device="cuda")

    def call(xv=hip.view(x), wp=w.data_ptr(), rv=hip.NULL_VIEW, yv=hip.view(y), dt=hip.F32, M=8, K=16, Nout=8, act=0):
        return L.ssr_linear(xv, wp, None, rv, yv, dt, M, K, Nout, act, hip.stream_ptr())

    assert call(dt=hip.BF16) == -2 and call(K=6) == -2 and call(Nout=6) == -2
    assert call(xv=hip.NULL_VIEW) == -1 and call(yv=hip.NULL_VIEW) == -1 and call(wp=None) == -1
    assert call(M=0) == -1 and call(K=0) == -1 and call(Nout=0) == -1 and call(act=4) == -1 and call(act=-1) == -1 and call(dt=9) == -1
    assert call(xv=hip.View(x.data_ptr(), 16, 4)) == -1 and call(yv=hip.View(y.data_ptr(), 8, 4)) == -1       # view narrower than its channels
    assert call(xv=hip.View(x.data_ptr() + 4, 16, 0)) == -1 and call(wp=w.data_ptr() + 4) == -1               # misaligned
    assert call(rv=hip.View(y.data_ptr(), 8, 4)) == -1 and call(yv=hip.View(y.data_ptr(), 6, 0), Nout=4) == -1
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                                            # no launch in any of these cases
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((y == 0.0).all())


# ------------------------------------------------------------------ ssr_layernorm_fwd
@pytest.mark.parametrize("rows", [1, 10, 729])
@pytest.mark.parametrize("C,eps", [(144, 1e-6), (768, 1e-5), (1152, 1e-6)])
def test_layernorm_matches_float64(C, eps, rows):
    """within the repository's exact-form rule for helper kernels, 2e-6 max|ref|; row 0 has a large mean and a small variance
    (1000 +- 0.01), the last row is constant (variance 0: the output is beta)"""
    from satlas_super_resolution_amd import hip
    g = torch.Generator().manual_seed(C + rows)
    x = torch.randn(rows, C, generator=g) * 3 + 0.5
    x[0] = 1000 + 0.01 * torch.randn(C, generator=g)
    if rows > 1:
        x[-1] = 2.5
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    want = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), eps)
    xb, gd, bd = _padded(x, C + 8, 4), gamma.cuda(), beta.cuda()
    y = torch.full((rows, C + 12), float("nan"), device="cuda")
    call = lambda xv, yv: hip.check(hip.lib().ssr_layernorm_fwd(xv, gd.data_ptr(), bd.data_ptr(), yv, hip.F32, rows, C, eps, hip.stream_ptr()),   # noqa: E731
                                    "ssr_layernorm_fwd")
    call(_V(xb, 4), _V(y, 8))
    got = y.cpu()
    assert bool(torch.isnan(torch.cat([got[:, :8], got[:, 8 + C:]], dim=-1)).all())
    err = float((got[:, 8:8 + C].double() - want).abs().max())
    print(f"ssr_layernorm_fwd C={C} rows={rows}: max |err| {err:.3e} = {err / float(want.abs().max()):.3e} max|ref|")
    assert err <= 2e-6 * float(want.abs().max())
    call(_V(xb, 4), _V(xb, 4))                                               # in place (the plan's ln_pre)
    assert torch.equal(xb.cpu()[:, 4:4 + C], got[:, 8:8 + C])


def test_layernorm_error_codes():
    from satlas_super_resolution_amd import hip
    L = hip.lib()
    x = torch.zeros(2, 16, device="cuda")
    y = torch.full((2, 16), 7.0, device="cuda")
    g = torch.ones(4096, device="cuda")
    big = torch.zeros(1, 4096, device="cuda")

    def call(xv=hip.view(x), yv=hip.view(y), gp=g.data_ptr(), dt=hip.F32, rows=2, C=16, eps=1e-6):
        return L.ssr_layernorm_fwd(xv, gp, g.data_ptr(), yv, dt, rows, C, eps, hip.stream_ptr())

    assert call(dt=hip.BF16) == -2 and call(C=6) == -2 and call(xv=hip.view(big), yv=hip.view(big), rows=1, C=2052) == -2
    assert call(xv=hip.NULL_VIEW) == -1 and call(yv=hip.NULL_VIEW) == -1 and call(gp=None) == -1
    assert call(rows=0) == -1 and call(C=0) == -1 and call(eps=-1.0) == -1 and call(yv=hip.View(y.data_ptr(), 16, 4)) == -1
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((y == 1.0).all())                                            # a constant row: beta


# ------------------------------------------------------------------ ssr_mha_fwd
MHA_CASES = [(10, 10, 2, 72), (197, 197, 2, 64), (729, 729, 2, 72), (1, 729, 2, 72), (1, 9, 2, 72)]


def _mha(q, k, v, N, Tq, Tk, heads, d):
    """q [N, Tq, C], k, v [N, Tk, C] on the host -> the whole output buffer [N Tq, C + 16] as numpy.  Self-attention shapes feed the
    three slices of ONE packed NaN-padded buffer; Tq != Tk feeds q from its own buffer and k, v from one packed buffer."""
    from satlas_super_resolution_amd import hip
    Cw = heads * d
    kv = torch.full((N * Tk, 3 * Cw + 8), float("nan"))
    kv[:, 4 + Cw:4 + 2 * Cw], kv[:, 4 + 2 * Cw:4 + 3 * Cw] = k.reshape(-1, Cw), v.reshape(-1, Cw)
    if Tq == Tk:
        kv[:, 4:4 + Cw] = q.reshape(-1, Cw)
        kv = kv.cuda()
        qv = _V(kv, 4)
    else:
        kv = kv.cuda()
        qb = _padded(q.reshape(-1, Cw), Cw + 8, 4)
        qv = _V(qb, 4)
    y = torch.full((N * Tq, Cw + 16), float("nan"), device="cuda")
    hip.check(hip.lib().ssr_mha_fwd(qv, _V(kv, 4 + Cw), _V(kv, 4 + 2 * Cw), _V(y, 8), hip.F32, N, Tq, Tk, heads, d, float(d) ** -0.5,
                                    hip.stream_ptr()), "ssr_mha_fwd")
    return y.cpu().numpy()


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("case", MHA_CASES, ids=["x".join(map(str, c)) for c in MHA_CASES])
def test_mha_matches_float64(case, N):
    """The tolerance is measured against the reference, not the kernel: the largest deviation of plain-torch fp32 attention on the
    CPU from the float64 one on the same inputs, over max|ref|; the device may deviate 4 x that (another summation order, expf) and
    never less than 2e-6 max|ref|.  Logits have a standard deviation of 2; query 0 of image 0 has a single dominant logit (softmax
    = one-hot to 1e-12) and the last query of the last image is zero (all logits equal: the mean of v)."""
    from satlas_super_resolution_amd import clipscore_metric as CM
    Tq, Tk, heads, d = case
    Cw = heads * d
    g = torch.Generator().manual_seed(Tq * 1000 + Tk + N)
    q, k, v = 2 * torch.randn(N, Tq, Cw, generator=g), torch.randn(N, Tk, Cw, generator=g), torch.randn(N, Tk, Cw, generator=g)
    q[0, 0] = 8 * k[0, Tk // 2]                                              # logit 8 |k|^2 / sqrt(d) ~ 8 sqrt(d) against N(0, 8^2 ...) others
    equal = (N > 1 or Tq > 1)
    if equal:
        q[-1, -1] = 0
    want = CM._attention(q.double(), k.double(), v.double(), heads)
    cpu32 = float((CM._attention(q, k, v, heads).double() - want).abs().max())
    ref = float(want.abs().max())
    gate = max(4 * cpu32, 2e-6 * ref)
    y1 = _mha(q, k, v, N, Tq, Tk, heads, d)
    got = torch.from_numpy(y1[:, 8:8 + Cw]).reshape(N, Tq, Cw).double()
    assert not torch.isnan(got).any() and np.isnan(np.delete(y1, np.s_[8:8 + Cw], axis=-1)).all()
    assert _mha(q, k, v, N, Tq, Tk, heads, d).tobytes() == y1.tobytes()      # a second launch: the same bytes
    last = _mha(q[-1:], k[-1:], v[-1:], 1, Tq, Tk, heads, d)
    assert last.tobytes() == y1[(N - 1) * Tq:].tobytes()                     # the last image alone: the same bytes as in the batch
    err = float((got - want).abs().max())
    print(f"ssr_mha_fwd Tq={Tq} Tk={Tk} heads={heads} d={d} N={N}: fp32 CPU deviation {cpu32 / ref:.3e} max|ref|, device {err / ref:.3e} max|ref| "
          f"(gate {gate / ref:.3e})")
    assert err <= gate, (err, gate)
    # the two special rows, stated on their own: one-hot picks v of that key, equal logits average v
    assert float((want[0, 0] - v[0, Tk // 2].double()).abs().max()) <= 1e-9
    assert float((got[0, 0] - v[0, Tk // 2].double()).abs().max()) <= gate
    if equal:
        assert float((got[-1, -1] - v[-1].double().mean(dim=0)).abs().max()) <= gate


def test_mha_error_codes():
    from satlas_super_resolution_amd import hip
    L = hip.lib()
    q = torch.zeros(4, 48, device="cuda")
    y = torch.full((4, 16), 7.0, device="cuda")

    def call(qv=hip.View(q.data_ptr(), 48, 0), kv=hip.View(q.data_ptr(), 48, 16), vv=hip.View(q.data_ptr(), 48, 32), yv=hip.view(y), dt=hip.F32,
             N=1, Tq=4, Tk=4, heads=2, d=8, scale=1.0):
        return L.ssr_mha_fwd(qv, kv, vv, yv, dt, N, Tq, Tk, heads, d, scale, hip.stream_ptr())

    assert call(dt=hip.BF16) == -2 and call(d=4, heads=4) == -2 and call(d=136, heads=1) == -2
    assert call(qv=hip.NULL_VIEW) == -1 and call(yv=hip.NULL_VIEW) == -1 and call(N=0) == -1 and call(Tq=0) == -1 and call(Tk=0) == -1
    assert call(heads=0) == -1 and call(d=0) == -1 and call(scale=float("nan")) == -1
    assert call(vv=hip.View(q.data_ptr(), 48, 36)) == -1 and call(yv=hip.View(y.data_ptr(), 16, 4)) == -1
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((y == 0.0).all())


# ------------------------------------------------------------------ ssr_vit_patch_input, ssr_vit_tokens, ssr_cosine_pairs
# (H, W, resized side, patch, grid): 384 = 27 * 14 + 6, the patch convolution drops the last 6 rows and columns
RESIZE_CASES = [(37, 53, 42, 14, 3), (128, 128, 224, 16, 14), (128, 128, 384, 14, 27), (500, 500, 224, 16, 14)]


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("bgr", [True, False])
@pytest.mark.parametrize("H,W,S,p,g", RESIZE_CASES)
def test_patch_input_is_bit_exact(H, W, S, p, g, bgr, normalize):
    """against the host gather: clip_resized_input in float32 (/ 255, then (x - mean) / std: one fp32 rounding per operation, IEEE
    division, no fused multiply-add) cut into patches in the column order of a patch-embedding weight [C, 3, p, p]"""
    import ctypes as C
    from satlas_super_resolution_amd import clipscore_metric as CM, hip
    N, fam = 2, "clip"
    u = torch.randint(0, 256, (N, H, W, 3), generator=torch.Generator().manual_seed(H + S), dtype=torch.uint8)
    x = CM.clip_resized_input(u, S, fam, bgr, normalize, torch.float32)[:, :, :g * p, :g * p]
    want = x.reshape(N, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(N * g * g, 3 * p * p).contiguous()
    rows, cols = (CM.nearest_index_table(n, S)[:g * p].to(torch.int32).cuda() for n in (H, W))
    y = torch.full((N * g * g, 3 * p * p + 12), float("nan"), device="cuda")
    perm = (C.c_int32 * 3)(*((2, 1, 0) if bgr else (0, 1, 2)))
    mean, std = ((C.c_float * 3)(*CM.CLIP_MEAN[fam]), (C.c_float * 3)(*CM.CLIP_STD[fam])) if normalize else (None, None)
    ud = u.cuda()
    hip.check(hip.lib().ssr_vit_patch_input(ud.data_ptr(), N, H, W, rows.data_ptr(), cols.data_ptr(), g, p, _V(y, 8), hip.F32, perm, mean, std,
                                            hip.stream_ptr()), "ssr_vit_patch_input")
    got = y.cpu()
    assert bool(torch.isnan(torch.cat([got[:, :8], got[:, 8 + 3 * p * p:]], dim=-1)).all())
    assert np.array_equal(got[:, 8:8 + 3 * p * p].numpy().view(np.uint32), want.numpy().view(np.uint32))


def test_patch_input_error_codes_and_bad_table():
    import ctypes as C
    from satlas_super_resolution_amd import hip
    L = hip.lib()
    u = torch.full((1, 4, 4, 3), 255, dtype=torch.uint8, device="cuda")
    idx = torch.tensor([0, 3, 4, -1], dtype=torch.int32, device="cuda")       # two entries outside the image
    y = torch.full((4, 12), 7.0, device="cuda")
    perm, bad = (C.c_int32 * 3)(0, 1, 2), (C.c_int32 * 3)(0, 1, 3)
    one = (C.c_float * 3)(1, 1, 1)

    def call(up=u.data_ptr(), ip=idx.data_ptr(), yv=hip.view(y), dt=hip.F32, N=1, H=4, W=4, g=2, p=2, pm=perm, mean=None, std=None):
        return L.ssr_vit_patch_input(up, N, H, W, ip, ip, g, p, yv, dt, pm, mean, std, hip.stream_ptr())

    assert call(dt=hip.BF16) == -2 and call(p=66) == -2
    assert call(up=None) == -1 and call(ip=None) == -1 and call(yv=hip.NULL_VIEW) == -1 and call(N=0) == -1 and call(g=0) == -1 and call(p=0) == -1
    assert call(pm=bad) == -1 and call(mean=one) == -1 and call(yv=hip.View(y.data_ptr(), 8, 0)) == -1
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert call() == 0
    got = y.cpu().reshape(2, 2, 3, 2, 2)                                      # [gy, gx, c, py, px]
    assert bool((got[0, 0] == 1).all()) and bool((got[1] == 0).all()) and bool((got[:, 1] == 0).all())      # entries outside the image: 0


@pytest.mark.parametrize("cls", [False, True])
def test_tokens_is_bit_exact(cls):
    from satlas_super_resolution_amd import hip
    N, G, Cw = 3, 9, 144
    g = torch.Generator().manual_seed(5)
    e, c, pos = torch.randn(N * G, Cw, generator=g), torch.randn(Cw, generator=g), torch.randn(G + cls, Cw, generator=g)
    rows = e.reshape(N, G, Cw)
    want = (torch.cat([c.expand(N, 1, Cw), rows], dim=1) if cls else rows) + pos
    eb, cd, pd = _padded(e, Cw + 8, 4), c.cuda(), pos.cuda()
    x = torch.full((N * (G + cls), Cw + 12), float("nan"), device="cuda")
    hip.check(hip.lib().ssr_vit_tokens(_V(eb, 4), cd.data_ptr() if cls else None, pd.data_ptr(), _V(x, 8), hip.F32, N, G, Cw, hip.stream_ptr()),
              "ssr_vit_tokens")
    got = x.cpu()
    assert bool(torch.isnan(torch.cat([got[:, :8], got[:, 8 + Cw:]], dim=-1)).all())
    assert torch.equal(got[:, 8:8 + Cw], want.reshape(-1, Cw))
    L = hip.lib()
    assert L.ssr_vit_tokens(_V(eb, 4), None, None, _V(x, 8), hip.F32, N, G, Cw, hip.stream_ptr()) == -1
    assert L.ssr_vit_tokens(_V(eb, 4), None, pd.data_ptr(), _V(x, 8), hip.BF16, N, G, Cw, hip.stream_ptr()) == -2
    assert L.ssr_vit_tokens(_V(eb, 4), None, pd.data_ptr(), _V(x, 8), hip.F32, N, G, 6, hip.stream_ptr()) == -2


@pytest.mark.parametrize("E", [32, 512, 1152])
def test_cosine_pairs_matches_float64(E):
    """sums in index order in fp64 of exact products: against the same sums in float64 within 4 * 2^-53 relative; identical vectors
    give 1 within 2^-50; a pair of zero vectors gives 0 (the 1e-8 clamp)"""
    from satlas_super_resolution_amd import hip
    N = 5
    g = torch.Generator().manual_seed(E)
    f = torch.randn(2, N, E, generator=g)
    f[1, 1] = f[0, 1]                                                        # identical
    f[1, 2] = f[0, 2] + 1e-3 * torch.randn(E, generator=g)                   # nearly identical
    f[:, 3] = 0
    a, b = f[0].double(), f[1].double()
    seq = lambda t: t.cumsum(dim=-1)[:, -1]                                  # noqa: E731  (cumsum adds in index order)
    want = seq(a * b) / (seq(a * a).sqrt() * seq(b * b).sqrt()).clamp_min(1e-8)
    fb = _padded(f.reshape(2 * N, E), E + 5, 3)                              # 4-byte alignment is enough
    out = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
    hip.check(hip.lib().ssr_cosine_pairs(_V(fb, 3), hip.F32, N, E, out.data_ptr(), hip.stream_ptr()), "ssr_cosine_pairs")
    got = out.cpu()
    rel = ((got - want).abs() / want.abs().clamp_min(1e-300))[[0, 1, 2, 4]]
    print(f"ssr_cosine_pairs E={E}: {got.tolist()}, max rel err {float(rel.max()):.3e}")
    assert float(rel.max()) <= 4 * 2.0 ** -53
    assert abs(1 - float(got[1])) <= 2.0 ** -50 and float(got[3]) == 0.0
    L = hip.lib()
    assert L.ssr_cosine_pairs(_V(fb, 3), hip.BF16, N, E, out.data_ptr(), hip.stream_ptr()) == -2
    assert L.ssr_cosine_pairs(_V(fb, 3), hip.F32, 0, E, out.data_ptr(), hip.stream_ptr()) == -1
    assert L.ssr_cosine_pairs(_V(fb, 3), hip.F32, N, E, None, hip.stream_ptr()) == -1
    assert L.ssr_cosine_pairs(_V(fb, 3), hip.F32, N, E + 4, out.data_ptr(), hip.stream_ptr()) == -1


# ------------------------------------------------------------------ the whole tower
FEEDS = {"reference": dict(bgr=True, normalize=False), "rgb+normalize": dict(bgr=False, normalize=True)}
TOWERS = {
    "siglip tiny": lambda: FX.tiny_state("siglip"),
    "clip tiny": lambda: FX.tiny_state("clip"),
    "siglip tiny, resized side 45 > 3 * 14": lambda: dict(FX.tiny_state("siglip"), image_size=torch.tensor(45)),
    "siglip full depth, width 144": lambda: FX.rule_state("siglip", 5, **dict(FX.TINY["siglip"], depth=27)),
    "siglip full width, 2 layers": lambda: FX.rule_state("siglip", 6, width=1152, heads=16, mlp=4304, depth=2, patch=14, grid=27),
    "clip ViT-B/16 full size": lambda: FX.rule_state("clip", 7, width=768, heads=12, mlp=3072, depth=12, patch=16, grid=14, out_dim=512),
}
@pytest.fixture(scope="module", params=list(TOWERS))
def tower(request):
    """one tower: its rule-filled state, the float64 and float32 CPU references of the three fixture images under both feeds
    (computed once), the gate they give the device - 4 x the largest deviation of the float32 CPU run of the project's own reference
    from its float64 run over ALL of these inputs - and the model on the device"""
    from satlas_super_resolution_amd import clipscore_metric as CM
    name = request.param
    state = TOWERS[name]()
    images = FX.fixture_images()
    ref, cpu32, top = {}, 0.0, 0.0
    for feed, kw in FEEDS.items():
        ref[feed] = CM.clip_image_features_reference(state, images, dtype=torch.float64, **kw)
        r32 = CM.clip_image_features_reference(state, images, dtype=torch.float32, **kw).double()
        cpu32, top = max(cpu32, float((r32 - ref[feed]).abs().max())), max(top, float(ref[feed].abs().max()))
    print(f"tower {name}: max|ref| {top:.3f}, fp32 CPU deviation {cpu32 / top:.3e} max|ref|; device gate {4 * cpu32 / top:.3e} max|ref|")
    return {"CM": CM, "name": name, "state": state, "images": images, "ref": ref, "cpu32": cpu32, "top": top, "gate": 4 * cpu32,
            "model": CM.CLIPVisualModel(state, "cuda")}


@pytest.mark.parametrize("feed", list(FEEDS))
def test_tower_features_match_reference(tower, feed):
    CM, images, want = tower["CM"], tower["images"], tower["ref"][feed]
    cfg = CM.vit_config_from_state(tower["state"])
    dev = images.cuda()
    got = CM.clip_image_features(dev, tower["model"], **FEEDS[feed])
    assert got.dtype == torch.float32 and got.shape == (images.shape[0], cfg["out_dim"]) and got.is_cuda
    err = float((got.cpu().double() - want).abs().max())
    print(f"tower {tower['name']} / {feed}: device {err / tower['top']:.3e} max|ref| (gate {tower['gate'] / tower['top']:.3e}, "
          f"fp32 CPU {tower['cpu32'] / tower['top']:.3e})")
    again = CM.clip_image_features(dev, tower["model"], **FEEDS[feed])
    assert got.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    assert err <= tower["gate"], (err, tower["gate"])
    tiny = tower["name"] in ("siglip tiny", "clip tiny")
    if tiny:                                                                 # the recorded values of the `transformers` classes
        gold = FX.load_golden(cfg["family"])
        assert torch.equal(gold["images"], images)
        assert float((got.cpu().double() - gold["features"][feed]).abs().max()) <= tower["gate"] + 1e-9 * tower["top"]
    # an image's features do not depend on the batch: alone, and first or last of three
    one = CM.clip_image_features(dev[:1], tower["model"], **FEEDS[feed])
    assert one.cpu().numpy().tobytes() == got[:1].cpu().numpy().tobytes()
    if tiny:
        three = CM.clip_image_features(torch.cat([dev[1:2], dev[2:3], dev[:1]]), tower["model"], **FEEDS[feed])
        assert three[2:].cpu().numpy().tobytes() == got[:1].cpu().numpy().tobytes() and three[:1].cpu().numpy().tobytes() == got[1:2].cpu().numpy().tobytes()


@pytest.mark.parametrize("feed", list(FEEDS))
def test_clipscore_pairs_match_reference(tower, feed):
    """the score of (image 0, image 1) and of (image 0, image 0): cos is 1-Lipschitz in each unit vector, so a feature error of at
    most e per element moves the score by at most 2 e sqrt(E) / min|f| (both vectors, worst direction)"""
    CM, images, ref = tower["CM"], tower["images"].cuda(), tower["ref"][feed]
    a, b = images[:1], images[1:2]
    want = CM.cosine_pairs_reference(ref[:1], ref[1:2])
    got = CM.clipscore(a, b, tower["model"], **FEEDS[feed])
    assert got.dtype == torch.float64 and got.shape == (1,) and not got.is_cuda
    E = ref.shape[1]
    bound = 2 * tower["gate"] * E ** 0.5 / float(ref.norm(dim=1).min())
    print(f"clipscore {tower['name']} / {feed}: {float(got[0])!r} against {float(want[0])!r}: |err| {abs(float(got[0] - want[0])):.3e} (bound {bound:.3e})")
    assert abs(float(got[0] - want[0])) <= bound
    same = CM.clipscore(a, a, tower["model"], **FEEDS[feed])
    assert abs(1 - float(same[0])) <= 2.0 ** -50


# ------------------------------------------------------------------ through the model plugin
def test_calculate_clipscore_through_the_test_pipeline(tmp_path, monkeypatch):
    """`test.metrics = {psnr, clipscore (siglip), clipscore_b16 (clip)}` over the s2naip_mini set with tiny towers saved in the
    packages' layouts (open_clip's with the visual.trunk. prefix, OpenAI's with visual.): each logged value is the mean of
    clipscore_reference over the written PNG pairs, within the tower gate propagated to the score; a second call gives the same
    bytes and loads nothing; esrgan_s2naip_urban.yml's own test.metrics block, given its weights files, runs all five metrics; without a
    weights file the same option file raises before the first image."""
    from PIL import Image
    from oracle import esrgan_oracle as O
    from satlas_super_resolution_amd import clipscore_metric as CM
    from satlas_super_resolution_amd.test import test_pipeline
    for env in CM.CLIP_ENV.values():
        monkeypatch.delenv(env, raising=False)
    monkeypatch.chdir(tmp_path)
    states = {"siglip": FX.tiny_state("siglip"), "clip": FX.tiny_state("clip")}
    torch.save(FX.to_timm_siglip(states["siglip"], "visual.trunk."), tmp_path / "siglip.pth")
    torch.save(FX.to_openai_clip(states["clip"]), tmp_path / "clip.pt")
    mini = os.path.join(GOLDEN, "s2naip_mini")
    g_kw = dict(num_in_ch=24, num_out_ch=3, scale=4, num_feat=64, num_block=1, num_grow_ch=32)
    gsd = O.generator_init(seed=5, **g_kw)
    torch.save({"params": gsd, "params_ema": gsd}, tmp_path / "net_g.pth")
    metrics = {"psnr": {"type": "calculate_psnr", "crop_border": 4, "test_y_channel": False},
               "clipscore": {"type": "calculate_clipscore", "clip_model": "siglip-ViT-SO400M-14", "clip_weights": str(tmp_path / "siglip.pth")},
               "clipscore_b16": {"type": "calculate_clipscore", "clip_model": "clip-ViT-B/16", "better": "higher",
                                 "clip_weights": str(tmp_path / "clip.pt")}}
    opt = {"name": "t", "model_type": "SSRESRGANModel", "scale": 4, "manual_seed": 0, "compute_dtype": "fp32x3",
           "test_datasets": {"test": {"name": "test", "type": "S2NAIPDataset", "phase": "test", "scale": 4, "n_s2_images": 8,
                                      "sentinel2_path": os.path.join(mini, "sentinel2"), "naip_path": os.path.join(mini, "naip")}},
           "network_g": dict(type="SSR_RRDBNet", **g_kw),
           "path": {"pretrain_network_g": str(tmp_path / "net_g.pth"), "param_key_g": "params_ema", "strict_load_g": True,
                    "visualization": str(tmp_path / "vis")},
           "test": {"save_img": True, "metrics": metrics}}
    loads = []
    real_load = CM.load_clip_visual_state
    monkeypatch.setattr(CM, "load_clip_visual_state", lambda *a, **k: (loads.append(a), real_load(*a, **k))[1])
    res = test_pipeline(opt, log=lambda *_: None)
    assert set(res) == {"test"} and set(res["test"]) == {"psnr", "clipscore", "clipscore_b16"}
    assert len(loads) == 2                                                   # once per tower, not once per image
    load = lambda f: torch.from_numpy(np.asarray(Image.open(tmp_path / "vis" / "test" / f)).copy())[None]        # noqa: E731
    sr = torch.cat([load(f"{i}_t.png") for i in range(5)])
    gt = torch.cat([load(f"{i}_t_gt.png") for i in range(5)])
    for name, fam in (("clipscore", "siglip"), ("clipscore_b16", "clip")):
        st = states[fam]
        f64 = [CM.clip_image_features_reference(st, t) for t in (sr, gt)]
        f32 = [CM.clip_image_features_reference(st, t, dtype=torch.float32).double() for t in (sr, gt)]
        gate = 4 * max(float((a - b).abs().max()) for a, b in zip(f32, f64))
        bound = 2 * gate * f64[0].shape[1] ** 0.5 / min(float(f.norm(dim=1).min()) for f in f64)
        want = float(CM.cosine_pairs_reference(*f64).mean())
        print(f"calculate_clipscore ({fam}) through the test pipeline: {res['test'][name]!r} against {want!r}: |err| {abs(res['test'][name] - want):.3e} "
              f"(bound {bound:.3e})")
        assert abs(res["test"][name] - want) <= bound
    assert abs(res["test"]["clipscore"] - res["test"]["clipscore_b16"]) > 1e-6
    # a second call of the entry on the same pair: the same bytes, nothing loaded (the pipeline itself is not rerun for this: the
    # generator's split-bf16 forward does not promise the same pixels twice)
    img, img2 = sr[0].cuda(), gt[0].cuda()
    for name in ("clipscore", "clipscore_b16"):
        first, second = M_clip(img, img2, metrics[name]), M_clip(img, img2, metrics[name])
        assert isinstance(first, float) and first == second and abs(1 - M_clip(img, img, metrics[name])) <= 2.0 ** -50
    assert len(loads) == 2
    # esrgan_s2naip_urban.yml's own test.metrics block, given its two weights files: all five metrics on the device
    import json
    import math
    from satlas_super_resolution_amd import lpips_metric as LM
    monkeypatch.delenv("SSR_LPIPS_WEIGHTS", raising=False)
    block = json.load(open(os.path.join(GOLDEN, "ssr_options.json")))["esrgan_s2naip_urban.yml"]["test"]["metrics"]
    torch.save(LM.lpips_random_state(17), tmp_path / "lpips_vgg.pth")
    block["clipscore"]["clip_weights"], block["lpips"]["lpips_weights"] = str(tmp_path / "siglip.pth"), str(tmp_path / "lpips_vgg.pth")
    five = test_pipeline(dict(opt, test={"save_img": False, "metrics": block}), log=lambda *_: None)["test"]
    assert set(five) == {"psnr", "ssim", "cpsnr", "lpips", "clipscore"} and all(math.isfinite(v) for v in five.values())
    assert five["lpips"] > 0 and abs(five["clipscore"] - res["test"]["clipscore"]) < 1e-2 and len(loads) == 2
    bad = dict(opt, test={"save_img": False, "metrics": {"clipscore": {"type": "calculate_clipscore", "clip_model": "siglip-ViT-SO400M-14"}}})
    with pytest.raises(NotImplementedError, match="SSR_CLIP_SIGLIP_WEIGHTS"):
        test_pipeline(bad, log=lambda *_: None)
    big = dict(opt, test={"save_img": False, "metrics": {"clipscore": {"type": "calculate_clipscore", "clip_model": "clipa-ViT-bigG-14"}}})
    with pytest.raises(NotImplementedError, match="clipa-ViT-bigG-14"):
        test_pipeline(big, log=lambda *_: None)


def M_clip(img, img2, entry):
    """one pair through the metric entry itself, as the model plugins call it"""
    from satlas_super_resolution_amd import metrics as M
    return M.METRICS["calculate_clipscore"](img, img2, **{k: v for k, v in entry.items() if k not in ("type", "better")})
