"""GPU: ssr_mha_mfma_fwd / ssr_mha_mfma_bwd (csrc/mha_mfma.hip; `tower_attention: mfma`) through the C ABI, held to what
ssr_mha_fwd / ssr_mha_bwd are held to in tests/test_gpu_clipscore.py (test_mha_matches_float64) and tests/test_gpu_clip_loss_kernels.py
(test_mha_bwd): the same inputs, the same float64 references (clipscore_metric._attention, clip_loss._attention_bwd) and the same
gates.  q, k and v are channel slices of one packed NaN-filled buffer, outputs are slices of NaN-filled buffers: an MFMA turns NaN * 0
into NaN, so a masked tail that multiplied something read by zero would show, as would anything written outside a view.

A block owns 128 rows and walks the other side 64 at a time: the shapes cross 64, 128 and 2 * 128 (65, 130, 197, 257, 729), sit below
a tile (9, 10, 81), and take the pooling shape Tq = 1.  The figures these tests printed on an MI355X are in
profiles/tower_attention_mfma/observed_errors.txt."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GATE = 1e-4          # tests/test_gpu_clip_loss_kernels.py: the project's bound for fp32-mode kernels, of max|ref|


def _V(t, coff=0):
    from satlas_super_resolution_amd import hip
    return hip.View(t.data_ptr(), t.shape[-1], coff)


def _padded(x2d, cs, coff):
    b = torch.full((x2d.shape[0], cs), float("nan"))
    b[:, coff:coff + x2d.shape[1]] = x2d
    return b.cuda()


# ------------------------------------------------------------------ forward
FWD_CASES = [(10, 10, 2, 72), (64, 64, 2, 64), (65, 65, 2, 64), (81, 81, 2, 64), (197, 197, 2, 64), (729, 729, 2, 72), (1, 9, 2, 72), (1, 81, 2, 64),
             (257, 257, 2, 64)]          # the last: 2 * 128 + 1, a third owner block of one row and a fifth key tile of one key


def _mha(q, k, v, N, Tq, Tk, heads, d):
    """_mha of tests/test_gpu_clipscore.py for the new entry -> the whole output buffer [N Tq, C + 16] as numpy"""
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
    hip.check(hip.lib().ssr_mha_mfma_fwd(qv, _V(kv, 4 + Cw), _V(kv, 4 + 2 * Cw), _V(y, 8), hip.F32, N, Tq, Tk, heads, d, float(d) ** -0.5,
                                         hip.stream_ptr()), "ssr_mha_mfma_fwd")
    return y.cpu().numpy()


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("case", FWD_CASES, ids=["x".join(map(str, c)) for c in FWD_CASES])
def test_mha_mfma_fwd_matches_float64(case, N):
    """The inputs, the two special rows (query 0 of image 0: one dominant logit; the last query of the last image: zero, all logits
    equal) and the gate of test_mha_matches_float64: max(4 x the deviation of plain-torch fp32 _attention on the CPU from float64,
    2e-6 max|ref|) - measured against the reference, not the kernel."""
    from satlas_super_resolution_amd import clipscore_metric as CM
    Tq, Tk, heads, d = case
    Cw = heads * d
    g = torch.Generator().manual_seed(Tq * 1000 + Tk + N)
    q, k, v = 2 * torch.randn(N, Tq, Cw, generator=g), torch.randn(N, Tk, Cw, generator=g), torch.randn(N, Tk, Cw, generator=g)
    q[0, 0] = 8 * k[0, Tk // 2]
    equal = (N > 1 or Tq > 1)
    if equal:
        q[-1, -1] = 0
    want = CM._attention(q.double(), k.double(), v.double(), heads)
    cpu32 = float((CM._attention(q, k, v, heads).double() - want).abs().max())
    ref = float(want.abs().max())
    gate = max(4 * cpu32, 2e-6 * ref)
    y1 = _mha(q, k, v, N, Tq, Tk, heads, d)
    got = torch.from_numpy(y1[:, 8:8 + Cw]).reshape(N, Tq, Cw).double()
    err = float((got - want).abs().max())
    print(f"ssr_mha_mfma_fwd Tq={Tq} Tk={Tk} heads={heads} d={d} N={N}: fp32 CPU deviation {cpu32 / ref:.3e} max|ref|, device {err / ref:.3e} "
          f"max|ref| (gate {gate / ref:.3e})")
    assert not torch.isnan(got).any() and np.isnan(np.delete(y1, np.s_[8:8 + Cw], axis=-1)).all()
    assert _mha(q, k, v, N, Tq, Tk, heads, d).tobytes() == y1.tobytes()      # a second launch: the same bytes
    last = _mha(q[-1:], k[-1:], v[-1:], 1, Tq, Tk, heads, d)
    assert last.tobytes() == y1[(N - 1) * Tq:].tobytes()                     # the last image alone: the same bytes as in the batch
    assert err <= gate, (err, gate)
    assert float((want[0, 0] - v[0, Tk // 2].double()).abs().max()) <= 1e-9
    assert float((got[0, 0] - v[0, Tk // 2].double()).abs().max()) <= gate
    if equal:
        assert float((got[-1, -1] - v[-1].double().mean(dim=0)).abs().max()) <= gate


# ------------------------------------------------------------------ backward
BWD_SHAPES = [(9, 9), (64, 64), (65, 65), (81, 81), (130, 130), (1, 81), (257, 257)]


@pytest.mark.parametrize("TqTk", BWD_SHAPES, ids=lambda t: f"{t[0]}x{t[1]}")
@pytest.mark.parametrize("d", [64, 72])
def test_mha_mfma_bwd(d, TqTk):
    """test_mha_bwd for the new entry: q, k, v are slices of one packed buffer, dq, dk, dv of another (the pooling case Tq = 1: q on its
    own, dq NULL); `want` is _attention_bwd in float64, cross-checked against autograd once per case"""
    from satlas_super_resolution_amd import hip
    from satlas_super_resolution_amd.clip_loss import _attention_bwd
    from satlas_super_resolution_amd.clipscore_metric import _attention
    Tq, Tk = TqTk
    N, heads = 2, 2
    Cw, pool = heads * d, Tq != Tk
    g = torch.Generator().manual_seed(d * 100 + Tq)
    q, k, v = torch.randn(N * Tq, Cw, generator=g) * 1.3, torch.randn(N * Tk, Cw, generator=g) * 1.3, torch.randn(N * Tk, Cw, generator=g)
    dy = torch.randn(N * Tq, Cw, generator=g)
    want = _attention_bwd(*(t.double().reshape(N, -1, Cw) for t in (q, k, v, dy)), heads)
    want = [t.reshape(-1, Cw) for t in want]
    qa, ka, va = (t.double().reshape(N, -1, Cw).requires_grad_(True) for t in (q, k, v))
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
    n_ws = int(L.ssr_mha_mfma_bwd_ws_floats(N, Tq, heads))
    assert n_ws == 3 * N * heads * Tq                                                 # include/ssr_hip.h: maximum, 1 / sum, delta per query row

    def run():
        ws = torch.full((n_ws + 8,), float("nan"), device="cuda")
        out = torch.full((N * Tk, 3 * Cw + 8), float("nan"), device="cuda")          # Tq == Tk unless pooling, where slice 0 stays unused
        dq = hip.NULL_VIEW if pool else _V(out, 4)
        hip.check(L.ssr_mha_mfma_bwd(*views, _V(dyb, 0), dq, _V(out, 4 + Cw), _V(out, 4 + 2 * Cw), ws.data_ptr(), hip.F32, N, Tq, Tk, heads, d,
                                     float(d) ** -0.5, hip.stream_ptr()), "ssr_mha_mfma_bwd")
        assert torch.isnan(ws[n_ws:]).all()                                           # the workspace beyond its size is untouched
        return out.cpu()

    o1, o2 = run(), run()
    errs = {}
    for i, name in enumerate(("dq", "dk", "dv")):
        if pool and i == 0:
            continue
        errs[name] = float((o1[:, 4 + i * Cw:4 + (i + 1) * Cw].double() - want[i]).abs().max() / want[i].abs().max())
        print(f"ssr_mha_mfma_bwd d={d} Tq={Tq} Tk={Tk} {name}: max |err| / max|ref| {errs[name]:.3e}")
    assert o1.numpy().tobytes() == o2.numpy().tobytes()
    assert torch.isnan(o1[:, :4]).all() and torch.isnan(o1[:, 4 + 3 * Cw:]).all()
    if pool:
        assert torch.isnan(o1[:, 4:4 + Cw]).all()                                     # a null dq: nothing written
    for name, err in errs.items():
        assert err <= GATE, name                                                      # NaN fails the comparison too


# ------------------------------------------------------------------ refusals launch nothing
def test_mha_mfma_fwd_error_codes():
    """the table of test_mha_error_codes, plus the head dims the FMA kernel takes and this one does not"""
    from satlas_super_resolution_amd import hip
    L = hip.lib()
    q = torch.zeros(4, 3 * 128, device="cuda")
    y = torch.full((4, 128), 7.0, device="cuda")

    def call(qv=hip.View(q.data_ptr(), 384, 0), kv=hip.View(q.data_ptr(), 384, 128), vv=hip.View(q.data_ptr(), 384, 256), yv=hip.view(y),
             dt=hip.F32, N=1, Tq=4, Tk=4, heads=2, d=64, scale=1.0):
        return L.ssr_mha_mfma_fwd(qv, kv, vv, yv, dt, N, Tq, Tk, heads, d, scale, hip.stream_ptr())

    assert call(dt=hip.BF16) == -2 and call(d=4, heads=4) == -2 and call(d=136, heads=1) == -2
    assert call(d=8, heads=2) == -2 and call(d=128, heads=1) == -2 and call(d=32, heads=4) == -2
    assert call(qv=hip.NULL_VIEW) == -1 and call(yv=hip.NULL_VIEW) == -1 and call(N=0) == -1 and call(Tq=0) == -1 and call(Tk=0) == -1
    assert call(heads=0) == -1 and call(d=0) == -1 and call(scale=float("nan")) == -1 and call(dt=9) == -1
    assert call(vv=hip.View(q.data_ptr(), 384, 260)) == -1 and call(yv=hip.View(y.data_ptr(), 128, 4)) == -1
    assert call(N=65536) == -2 and call(Tk=(1 << 20) + 1) == -2
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((y == 0.0).all())


def test_mha_mfma_bwd_error_codes():
    from satlas_super_resolution_amd import hip
    L, st = hip.lib(), hip.stream_ptr()
    a = torch.zeros(8, 128, device="cuda")
    o = torch.full((8, 128), 7.0, device="cuda")
    o2 = torch.full((8, 128), 7.0, device="cuda")
    ws = torch.full((64,), 7.0, device="cuda")
    va, vo, vo2, NV = hip.view(a), hip.view(o), hip.view(o2), hip.NULL_VIEW

    def mha(**k):
        return L.ssr_mha_mfma_bwd(k.get("q", va), va, va, k.get("dy", va), k.get("dq", NV), k.get("dk", vo), vo2, k.get("ws", ws.data_ptr()),
                                  k.get("dt", hip.F32), k.get("N", 1), k.get("Tq", 8), k.get("Tk", 8), k.get("heads", 2), k.get("d", 64),
                                  k.get("scale", 0.125), st)

    assert mha(d=32) == -2 and mha(d=128) == -2 and mha(d=8) == -2 and mha(dt=hip.BF16) == -2 and mha(N=65536) == -2
    assert mha(ws=None) == -1 and mha(Tq=0) == -1 and mha(Tk=0) == -1 and mha(N=0) == -1 and mha(q=NV) == -1 and mha(dy=NV) == -1
    assert mha(dk=NV) == -1 and mha(heads=3) == -1 and mha(heads=0) == -1 and mha(d=0) == -1 and mha(dt=9) == -1
    assert mha(scale=float("nan")) == -1 and mha(dq=hip.View(o.data_ptr(), 128, 4)) == -1 and mha(ws=ws.data_ptr() + 2) == -1
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and bool((o2 == 7.0).all()) and bool((ws == 7.0).all())
    assert mha() == 0                                                                  # zeros in: dk = dv = 0
    torch.cuda.synchronize()
    assert bool((o == 0.0).all()) and bool((o2 == 0.0).all())
