"""GPU: the C-ABI entries of csrc/vit_bwd.hip (the tower's backward pass for the CLIP loss of train.clip_opt), each against a float64
restatement of what include/ssr_hip.h says it computes.  The gate is the project's bound for fp32-mode kernels, 1e-4 of max|ref|;
every kernel must also give identical bytes on a second launch.  Operands are channel slices of wider NaN-filled buffers: nothing
outside a view is read or written.  The figures these tests printed on an MI355X are in profiles/clip_loss/observed_errors.txt."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GATE = 1e-4


def _padded(x2d, cs, coff, fill=float("nan")):
    """x [rows, c] -> a buffer [rows, cs] holding x at channel coff, on the device"""
    b = torch.full((x2d.shape[0], cs), fill)
    b[:, coff:coff + x2d.shape[1]] = x2d
    return b.cuda()


def _V(t, coff=0):
    from satlas_super_resolution_amd import hip
    return hip.View(t.data_ptr(), t.shape[-1], coff)


def _rel(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


# ------------------------------------------------------------------ ssr_layernorm_bwd
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("rows", [1, 7, 130])
@pytest.mark.parametrize("C_", [128, 144])
def test_layernorm_bwd(C_, rows, residual):
    from satlas_super_resolution_amd import hip
    g = torch.Generator().manual_seed(C_ * 1000 + rows)
    x = torch.randn(rows, C_, generator=g) * 2 + 3
    gamma, dy, r = 1 + 0.2 * torch.randn(C_, generator=g), torch.randn(rows, C_, generator=g), torch.randn(rows, C_, generator=g)
    eps = 1e-6
    x64 = x.double().requires_grad_(True)
    F.layer_norm(x64, (C_,), gamma.double(), torch.zeros(C_, dtype=torch.float64), eps).backward(dy.double())
    want = x64.grad + (r.double() if residual else 0)
    xb, dyb, rb, gd = _padded(x, C_ + 8, 4), _padded(dy, C_ + 4, 0), _padded(r, C_ + 12, 8), gamma.cuda()

    def run():
        out = torch.full((rows, C_ + 8), float("nan"), device="cuda")
        hip.check(hip.lib().ssr_layernorm_bwd(_V(xb, 4), gd.data_ptr(), _V(dyb, 0), _V(rb, 8) if residual else hip.NULL_VIEW, _V(out, 4), hip.F32,
                                              rows, C_, eps, hip.stream_ptr()), "ssr_layernorm_bwd")
        return out.cpu()

    o1, o2 = run(), run()
    assert o1.numpy().tobytes() == o2.numpy().tobytes()
    assert torch.isnan(o1[:, :4]).all() and torch.isnan(o1[:, 4 + C_:]).all() and not torch.isnan(o1[:, 4:4 + C_]).any()
    err = _rel(o1[:, 4:4 + C_], want)
    print(f"ssr_layernorm_bwd C={C_} rows={rows} residual={residual}: max |err| / max|ref| {err:.3e}")
    assert err <= GATE
    # in place over dy: everything is read before the first store
    dyc = dyb.clone()
    hip.check(hip.lib().ssr_layernorm_bwd(_V(xb, 4), gd.data_ptr(), _V(dyc, 0), _V(rb, 8) if residual else hip.NULL_VIEW, _V(dyc, 0), hip.F32,
                                          rows, C_, eps, hip.stream_ptr()), "ssr_layernorm_bwd in place")
    assert dyc[:, :C_].cpu().numpy().tobytes() == o1[:, 4:4 + C_].contiguous().numpy().tobytes()


# ------------------------------------------------------------------ the activation passes
ACT_NAMES = ("quick_gelu", "gelu_tanh", "gelu_erf")
ACTS = {"quick_gelu": lambda v: v * torch.sigmoid(1.702 * v), "gelu_tanh": lambda v: F.gelu(v, approximate="tanh"), "gelu_erf": lambda v: F.gelu(v)}


@pytest.mark.parametrize("act", ACT_NAMES + ("none",))
def test_act_fwd_gives_the_fused_activation_bytes(act):
    """ssr_linear with SSR_VIT_ACT_NONE followed by ssr_vit_act_fwd == ssr_linear with the activation fused, byte for byte"""
    from satlas_super_resolution_amd import hip
    M, K, Nout = 70, 144, 200
    g = torch.Generator().manual_seed(3)
    x, w, b = _padded(torch.randn(M, K, generator=g), K + 8, 4), (torch.randn(Nout, K, generator=g) / K ** 0.5).cuda(), torch.randn(Nout, generator=g).cuda()
    L, st = hip.lib(), hip.stream_ptr()
    fused, pre = (torch.full((M, Nout + 8), float("nan"), device="cuda") for _ in range(2))
    hip.check(L.ssr_linear(_V(x, 4), w.data_ptr(), b.data_ptr(), hip.NULL_VIEW, _V(fused, 4), hip.F32, M, K, Nout, hip.VIT_ACTS[act], st), "fused")
    hip.check(L.ssr_linear(_V(x, 4), w.data_ptr(), b.data_ptr(), hip.NULL_VIEW, _V(pre, 4), hip.F32, M, K, Nout, 0, st), "pre")
    post = torch.full((M, Nout + 16), float("nan"), device="cuda")
    hip.check(L.ssr_vit_act_fwd(_V(pre, 4), _V(post, 8), hip.F32, M, Nout, hip.VIT_ACTS[act], st), "ssr_vit_act_fwd")
    assert post[:, 8:8 + Nout].cpu().numpy().tobytes() == fused[:, 4:4 + Nout].cpu().numpy().tobytes()
    assert torch.isnan(post[:, :8]).all() and torch.isnan(post[:, 8 + Nout:]).all()
    hip.check(L.ssr_vit_act_fwd(_V(pre, 4), _V(pre, 4), hip.F32, M, Nout, hip.VIT_ACTS[act], st), "in place")
    assert pre.cpu().numpy().tobytes() == fused.cpu().numpy().tobytes()


@pytest.mark.parametrize("act", ACT_NAMES)
def test_act_bwd(act):
    from satlas_super_resolution_amd import hip
    rows, C_ = 37, 200
    g = torch.Generator().manual_seed(5)
    pre = torch.randn(rows, C_, generator=g) * 2.5
    pre[0, :8] = torch.tensor([0.0, -0.0, 8.0, -8.0, 1e-4, -1e-4, 20.0, -20.0])
    dpost = torch.randn(rows, C_, generator=g)
    p64 = pre.double().requires_grad_(True)
    ACTS[act](p64).backward(dpost.double())
    pb, gb = _padded(pre, C_ + 8, 4), _padded(dpost, C_ + 4, 4)

    def run():
        out = torch.full((rows, C_ + 8), float("nan"), device="cuda")
        hip.check(hip.lib().ssr_vit_act_bwd(_V(pb, 4), _V(gb, 4), _V(out, 0), hip.F32, rows, C_, hip.VIT_ACTS[act], hip.stream_ptr()), "ssr_vit_act_bwd")
        return out.cpu()

    o1, o2 = run(), run()
    assert o1.numpy().tobytes() == o2.numpy().tobytes()
    assert torch.isnan(o1[:, C_:]).all()
    err = _rel(o1[:, :C_], p64.grad)
    print(f"ssr_vit_act_bwd {act}: max |err| / max|ref| {err:.3e}")
    assert err <= GATE


# ------------------------------------------------------------------ ssr_mha_bwd
@pytest.mark.parametrize("TqTk", [(9, 9), (64, 64), (65, 65), (81, 81), (1, 81)], ids=lambda t: f"{t[0]}x{t[1]}")
@pytest.mark.parametrize("d", [64, 72])
def test_mha_bwd(d, TqTk):
    """q, k, v are slices of one packed buffer, dq, dk, dv of another (the pooling case Tq = 1: q on its own, dq NULL)"""
    from satlas_super_resolution_amd import hip
    from satlas_super_resolution_amd.clip_loss import _attention_bwd
    Tq, Tk = TqTk
    N, heads = 2, 2
    Cw, pool = heads * d, Tq != Tk
    g = torch.Generator().manual_seed(d * 100 + Tq)
    q, k, v = torch.randn(N * Tq, Cw, generator=g) * 1.3, torch.randn(N * Tk, Cw, generator=g) * 1.3, torch.randn(N * Tk, Cw, generator=g)
    dy = torch.randn(N * Tq, Cw, generator=g)
    want = _attention_bwd(*(t.double().reshape(N, -1, Cw) for t in (q, k, v, dy)), heads)
    want = [t.reshape(-1, Cw) for t in want]
    # cross-check the restatement against autograd once per case
    qa, ka, va = (t.double().reshape(N, -1, Cw).requires_grad_(True) for t in (q, k, v))
    from satlas_super_resolution_amd.clipscore_metric import _attention
    _attention(qa, ka, va, heads).backward(dy.double().reshape(N, Tq, Cw))
    for a, b in zip((qa, ka, va), want):
        assert float((a.grad.reshape(-1, Cw) - b).abs().max()) <= 1e-12 * float(b.abs().max()) + 1e-300
    if pool:
        qb = _padded(q, Cw + 8, 4)
        kvb = torch.full((N * Tk, 2 * Cw + 8), float("nan"))
        kvb[:, 4:4 + Cw], kvb[:, 4 + Cw:4 + 2 * Cw] = k, v
        kvb = kvb.cuda()
        views = [_V(qb, 4), _V(kvb, 4), _V(kvb, 4 + Cw)]
    else:
        pk = torch.full((N * Tq, 3 * Cw + 8), float("nan"))
        pk[:, 4:4 + Cw], pk[:, 4 + Cw:4 + 2 * Cw], pk[:, 4 + 2 * Cw:4 + 3 * Cw] = q, k, v
        pk = pk.cuda()
        views = [_V(pk, 4 + i * Cw) for i in range(3)]
    dyb = _padded(dy, Cw + 4, 0)
    L = hip.lib()
    n_ws = int(L.ssr_mha_bwd_ws_floats(N, Tq, heads))
    assert n_ws == 3 * N * heads * Tq

    def run():
        ws = torch.full((n_ws + 8,), float("nan"), device="cuda")
        out = torch.full((N * Tk, 3 * Cw + 8), float("nan"), device="cuda")          # Tq == Tk unless pooling, where slice 0 stays unused
        dq = hip.NULL_VIEW if pool else _V(out, 4)
        hip.check(L.ssr_mha_bwd(*views, _V(dyb, 0), dq, _V(out, 4 + Cw), _V(out, 4 + 2 * Cw), ws.data_ptr(), hip.F32, N, Tq, Tk, heads, d,
                                float(d) ** -0.5, hip.stream_ptr()), "ssr_mha_bwd")
        assert torch.isnan(ws[n_ws:]).all() and not torch.isnan(ws[:n_ws]).any()
        return out.cpu()

    o1, o2 = run(), run()
    assert o1.numpy().tobytes() == o2.numpy().tobytes()
    assert torch.isnan(o1[:, :4]).all() and torch.isnan(o1[:, 4 + 3 * Cw:]).all()
    if pool:
        assert torch.isnan(o1[:, 4:4 + Cw]).all()                                     # a null dq: nothing written
    for i, name in enumerate(("dq", "dk", "dv")):
        if pool and i == 0:
            continue
        err = _rel(o1[:, 4 + i * Cw:4 + (i + 1) * Cw], want[i])
        print(f"ssr_mha_bwd d={d} Tq={Tq} Tk={Tk} {name}: max |err| / max|ref| {err:.3e}")
        assert err <= GATE, name


# ------------------------------------------------------------------ the input pair
OPENAI_MEAN, OPENAI_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


@pytest.mark.parametrize("HW", [(5, 7), (100, 60)], ids=lambda t: f"{t[0]}x{t[1]}")
@pytest.mark.parametrize("perm", [(0, 1, 2), (2, 0, 1)], ids=["rgb", "perm201"])
def test_float_input_pair(HW, perm):
    """48 x 48 resized image, patch 8, grid 5: the patch matrix holds the first 40 rows and columns, the last 8 carry no gradient.
    Forward: with the float image (float)u / 255.0f (IEEE division, what torch's true division gives) the bytes are those of
    ssr_vit_patch_input on u - the order of both kernels is [/ 255,] (v - mean) / std with one rounding per step.
    Backward: the exact transpose, ADDED to the prior content of channels coff .. coff + 2 of an 8-channel gradient image."""
    from satlas_super_resolution_amd import hip
    from satlas_super_resolution_amd.clip_loss import nearest_inverse_ranges
    from satlas_super_resolution_amd.clipscore_metric import nearest_index_table
    H, W = HW
    N, S, p, grid = 2, 48, 8, 5
    gp, KP = grid * p, 3 * p * p
    g = torch.Generator().manual_seed(H)
    u8 = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    img = torch.full((N, H, W, 8), float("nan"))
    img[..., 4:7] = u8.float() / 255
    imgd, u8d = img.cuda(), u8.cuda()
    L, st = hip.lib(), hip.stream_ptr()
    rowt, colt = nearest_index_table(H, S), nearest_index_table(W, S)
    rowidx, colidx = rowt[:gp].to(torch.int32).cuda(), colt[:gp].to(torch.int32).cuda()
    cperm, cmean, cstd = (C.c_int32 * 3)(*perm), (C.c_float * 3)(*OPENAI_MEAN), (C.c_float * 3)(*OPENAI_STD)
    want_b, got_b = (torch.full((N * grid * grid, KP + 8), float("nan"), device="cuda") for _ in range(2))
    hip.check(L.ssr_vit_patch_input(u8d.data_ptr(), N, H, W, rowidx.data_ptr(), colidx.data_ptr(), grid, p, _V(want_b, 4), hip.F32, cperm, cmean,
                                    cstd, st), "ssr_vit_patch_input")
    hip.check(L.ssr_vit_float_input(hip.View(imgd.data_ptr(), 8, 4), N, H, W, rowidx.data_ptr(), colidx.data_ptr(), grid, p, _V(got_b, 4), hip.F32,
                                    cperm, cmean, cstd, st), "ssr_vit_float_input")
    assert got_b.cpu().numpy().tobytes() == want_b.cpu().numpy().tobytes()
    # and against the definition: x = (img[rows][cols][perm] - mean) / std in float64
    mean, std = (torch.tensor(t, dtype=torch.float32).double() for t in (OPENAI_MEAN, OPENAI_STD))
    x64 = (img[..., 4:7].double()[:, rowt[:gp]][:, :, colt[:gp]][..., list(perm)] - mean) / std                  # [N, gp, gp, 3]
    want_patch = x64.reshape(N, grid, p, grid, p, 3).permute(0, 1, 3, 5, 2, 4).reshape(N * grid * grid, KP)
    assert _rel(got_b[:, 4:4 + KP], want_patch) <= 2 ** -22

    # backward
    dpatch = torch.randn(N * grid * grid, KP, generator=g)
    dpb = _padded(dpatch, KP + 8, 4)
    prior = torch.randn(N, H, W, 8, generator=g)
    rr, cr = nearest_inverse_ranges(H, S, gp), nearest_inverse_ranges(W, S, gp)
    dx = dpatch.double().reshape(N, grid, grid, 3, p, p).permute(0, 1, 4, 2, 5, 3).reshape(N, gp, gp, 3)           # [N, Y, X, c]
    want = prior.double().clone()
    scat = torch.zeros(N, H, W, 3, dtype=torch.float64)
    scat.index_put_((torch.arange(N)[:, None, None], rowt[:gp][None, :, None], colt[:gp][None, None, :]), dx / std, accumulate=True)
    for c in range(3):
        want[..., 4 + perm[c]] += scat[..., c]
    rrd, crd = rr.to(torch.int32).cuda(), cr.to(torch.int32).cuda()

    def run():
        gimg = prior.cuda()
        hip.check(L.ssr_vit_float_input_bwd(_V(dpb, 4), N, H, W, rrd.data_ptr(), crd.data_ptr(), grid, p, hip.View(gimg.data_ptr(), 8, 4), hip.F32,
                                            cperm, cstd, st), "ssr_vit_float_input_bwd")
        return gimg.cpu()

    o1, o2 = run(), run()
    assert o1.numpy().tobytes() == o2.numpy().tobytes()
    other = [0, 1, 2, 3, 7]
    assert o1[..., other].numpy().tobytes() == prior[..., other].contiguous().numpy().tobytes()                      # other channels untouched
    err = _rel(o1[..., 4:7], want[..., 4:7])
    print(f"ssr_vit_float_input_bwd {H}x{W} perm={perm}: max |err| / max|ref| {err:.3e}")
    assert err <= GATE
    if H == 100:                                                                # sources that nothing reads keep their prior content
        unread = (rr[:, 1] == rr[:, 0])
        assert bool(unread.any()) and o1[:, unread][..., 4:7].numpy().tobytes() == prior[:, unread][..., 4:7].contiguous().numpy().tobytes()


# ------------------------------------------------------------------ ssr_feature_l1
def test_feature_l1():
    """B E = 3 * 100 = 300 is no multiple of the 256-thread block; two exact-zero differences give a zero gradient"""
    from satlas_super_resolution_amd import hip
    B, E, weight = 3, 100, 0.75
    g = torch.Generator().manual_seed(2)
    fx, fg = torch.randn(B, E, generator=g), torch.randn(B, E, generator=g)
    fg[0, 0], fg[2, 99] = fx[0, 0], fx[2, 99]
    d = fx.double() - fg.double()
    want_loss, want_grad = weight * d.abs().mean(), weight * torch.sign(d) / (B * E)
    fxb, fgb = _padded(fx, E + 4, 4), _padded(fg, E + 8, 0)

    def run(flags):
        loss = torch.full((hip.LOSS_SLOTS,), 0.0, device="cuda")
        loss[0] = 1.5                                                           # the scalar is ADDED to
        grad = torch.full((B, E + 8), float("nan"), device="cuda")
        hip.check(hip.lib().ssr_feature_l1(_V(fxb, 4), _V(fgb, 0), _V(grad, 4), B, E, weight, loss.data_ptr(), flags, hip.stream_ptr()), "ssr_feature_l1")
        return loss.cpu(), grad.cpu()

    (l1, g1), (l2, g2), (l3, g3) = run(0), run(0), run(hip.DETERMINISTIC)
    assert l1.numpy().tobytes() == l2.numpy().tobytes() == l3.numpy().tobytes() and g1.numpy().tobytes() == g2.numpy().tobytes() == g3.numpy().tobytes()
    assert bool((l1[1:] == 0).all()) and torch.isnan(g1[:, :4]).all() and torch.isnan(g1[:, 4 + E:]).all()
    got = g1[:, 4:4 + E]
    assert float(got[0, 0]) == 0.0 and float(got[2, 99]) == 0.0
    el, eg = abs(float(l1[0]) - 1.5 - float(want_loss)) / float(want_loss), _rel(got, want_grad)
    print(f"ssr_feature_l1: loss |err| / ref {el:.3e}, gradient max |err| / max|ref| {eg:.3e}")
    assert el <= GATE and eg <= GATE


# ------------------------------------------------------------------ refusals launch nothing
def test_error_codes_launch_nothing():
    from satlas_super_resolution_amd import hip
    L, st = hip.lib(), hip.stream_ptr()
    a = torch.full((8, 128), 7.0, device="cuda")
    o = torch.full((8, 128), 7.0, device="cuda")
    w = torch.ones(128, device="cuda")
    va, vo, NV = hip.view(a), hip.view(o), hip.NULL_VIEW
    assert L.ssr_layernorm_bwd(va, w.data_ptr(), va, NV, vo, hip.BF16, 8, 128, 1e-6, st) == -2
    assert L.ssr_layernorm_bwd(va, w.data_ptr(), va, NV, vo, hip.F32, 8, 126, 1e-6, st) == -2
    assert L.ssr_layernorm_bwd(va, None, va, NV, vo, hip.F32, 8, 128, 1e-6, st) == -1
    assert L.ssr_layernorm_bwd(va, w.data_ptr(), NV, NV, vo, hip.F32, 8, 128, 1e-6, st) == -1
    assert L.ssr_layernorm_bwd(va, w.data_ptr(), va, NV, vo, hip.F32, 0, 128, 1e-6, st) == -1
    assert L.ssr_layernorm_bwd(va, w.data_ptr(), va, NV, hip.View(o.data_ptr(), 128, 4), hip.F32, 8, 128, 1e-6, st) == -1
    assert L.ssr_vit_act_fwd(va, vo, hip.F32, 8, 128, 4, st) == -1 and L.ssr_vit_act_fwd(va, vo, hip.F32, 8, 126, 2, st) == -2
    assert L.ssr_vit_act_fwd(NV, vo, hip.F32, 8, 128, 2, st) == -1 and L.ssr_vit_act_bwd(va, NV, vo, hip.F32, 8, 128, 2, st) == -1
    assert L.ssr_vit_act_bwd(va, va, vo, hip.BF16, 8, 128, 2, st) == -2
    ws = torch.zeros(64, device="cuda")
    mha = lambda **k: L.ssr_mha_bwd(k.get("q", va), va, va, va, NV, vo, vo, k.get("ws", ws.data_ptr()), k.get("dt", hip.F32), 1, k.get("Tq", 8), 8,   # noqa: E731
                                    k.get("heads", 2), k.get("d", 64), 0.125, st)
    assert mha(d=32) == -2 and mha(d=128) == -2 and mha(dt=hip.BF16) == -2
    assert mha(ws=None) == -1 and mha(Tq=0) == -1 and mha(q=NV) == -1 and mha(heads=3) == -1 and mha(dt=9) == -1
    loss = torch.full((4,), 7.0, device="cuda")
    assert L.ssr_feature_l1(va, va, vo, 8, 128, 1.0, None, 0, st) == -1 and L.ssr_feature_l1(va, va, vo, 8, 128, 1.0, loss.data_ptr(), 3, st) == -1
    assert L.ssr_feature_l1(va, NV, vo, 8, 128, 1.0, loss.data_ptr(), 0, st) == -1 and L.ssr_feature_l1(va, va, vo, 0, 128, 1.0, loss.data_ptr(), 0, st) == -1
    idx = torch.zeros(64, dtype=torch.int32, device="cuda")
    perm, bad, std = (C.c_int32 * 3)(0, 1, 2), (C.c_int32 * 3)(0, 0, 2), (C.c_float * 3)(1, 1, 1)
    img = hip.View(a.data_ptr(), 8, 0)
    fin = lambda **k: L.ssr_vit_float_input(k.get("img", img), 1, 4, 4, idx.data_ptr(), idx.data_ptr(), 1, k.get("p", 2), vo, k.get("dt", hip.F32),  # noqa: E731
                                            k.get("perm", perm), None, None, st)
    assert fin(perm=bad) == -1 and fin(img=NV) == -1 and fin(p=66) == -2 and fin(dt=hip.BF16) == -2 and fin(p=8) == -1       # 3 * 64 channels > the view's 128
    assert L.ssr_vit_float_input_bwd(va, 1, 4, 4, idx.data_ptr(), idx.data_ptr(), 1, 2, hip.View(o.data_ptr(), 8, 0), hip.F32, bad, std, st) == -1
    assert L.ssr_vit_float_input_bwd(va, 1, 4, 4, None, idx.data_ptr(), 1, 2, hip.View(o.data_ptr(), 8, 0), hip.F32, perm, std, st) == -1
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and bool((loss == 7.0).all())
