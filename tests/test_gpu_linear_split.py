"""GPU: ssr_linear_split and ssr_linear_split_pack (csrc/linear_split.hip) on their own, for both piece encodings.

Held to two references.  The ARITHMETIC MODEL, linear_split.linear_split_reference (the three piece products in float64): the kernel
forms the same pieces (round to nearest, as torch's .half() / .bfloat16()) and multiplies them exactly (two 11-bit or 8-bit significands
give at most 22 bits: exact in fp32), so all that separates the two before the activation is the fp32 summation of 3 K exact products
and the bias, in whatever order:

    |err_pre| <= gamma_(3K+1) (sum_k |x_hi w_hi| + |x_hi w_lo| + |x_lo w_hi| + |b|) + K 2^-126,   gamma_n = n u / (1 - n u), u = 2^-24

(K 2^-126 covers products or a rescaled sum that land in fp32's subnormals).  And the FLOAT64 PRODUCT, within that plus
linear_split.split_representation_bound (what the pieces drop; derived and checked on the CPU in tests/test_linear_split_host.py).
After the activation both follow test_linear_matches_float64 of tests/test_gpu_clipscore.py: the bound times the activation's
Lipschitz constant, plus 4 x the deviation of torch's fp32 CPU activation from the float64 one on the same pre-activations, plus one
rounding of the result for the residual.  Nothing in a tolerance comes from what the kernel returns.

Inputs and outputs are channel slices of wider NaN-filled buffers: nothing outside X[M, K] is read (no NaN comes out), nothing outside
Y[M, Nout] is written.  The figures these tests printed on an MI355X are in profiles/clip_loss_split/observed_errors.txt."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_clipscore import ACTS, LINEAR_VARIANTS, LIPSCHITZ, U32, _padded, _V

pytestmark = pytest.mark.gpu

# a single row; a K tail inside one MFMA group; K no multiple of 16 and tiles masked in M and Nout; K = 588 (patch 14) over more than
# one block in M and Nout; one real layer width
SHAPES = [(1, 4, 4), (5, 20, 12), (33, 200, 68), (130, 588, 132), (64, 768, 256)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
PIECES = ("f16", "bf16")


def _code(pieces):
    from satlas_super_resolution_amd import hip
    return {"f16": hip.SPLIT_F16, "bf16": hip.SPLIT_BF16}[pieces]


@functools.lru_cache(maxsize=None)
def _case(M, K, Nout, pieces, xscale=1.0):
    """inputs, the model's and the exact pre-bias products and both bounds' sums of one shape, computed once for all its variants"""
    from satlas_super_resolution_amd import linear_split as S
    g = torch.Generator().manual_seed(M * 7919 + K * 31 + Nout)
    x, w = torch.randn(M, K, generator=g) * xscale, torch.randn(Nout, K, generator=g) / K ** 0.5
    b, r = torch.randn(Nout, generator=g), torch.randn(M, Nout, generator=g)
    assert float(x.abs().max()) < 65504 and float(w.abs().max()) < 64
    return (x, w, b, r, S.linear_split_reference(x, w, None, pieces), S.split_piece_magnitude(x, w, pieces),
            x.double() @ w.double().t(), S.split_representation_bound(x, w, pieces))


def _linear(pieces, x, w, b, r, M, K, Nout, act, in_place, rows=None):
    """-> the whole output buffer [rows, Nout + 16] (NaN outside the slice at channel 8) as numpy"""
    from satlas_super_resolution_amd import hip
    from satlas_super_resolution_amd.linear_split import pack_split_weight
    rows = rows or M
    xb, wpk = _padded(x[:rows], K + 8, 4), pack_split_weight(w.cuda(), _code(pieces))
    bd = b.cuda() if b is not None else None
    y = torch.full((rows, Nout + 16), float("nan"), device="cuda")
    rv, keep = hip.NULL_VIEW, None
    if r is not None and in_place:
        y[:, 8:8 + Nout] = r[:rows].cuda()
        rv = _V(y, 8)
    elif r is not None:
        keep = _padded(r[:rows], Nout + 12, 4)
        rv = _V(keep, 4)
    hip.check(hip.lib().ssr_linear_split(_V(xb, 4), wpk.data_ptr(), bd.data_ptr() if bd is not None else None, rv, _V(y, 8), _code(pieces),
                                         rows, K, Nout, hip.VIT_ACTS[act], hip.stream_ptr()), "ssr_linear_split")
    return y.cpu().numpy()


def _check(case, pieces, variant, xscale=1.0):
    M, K, Nout = case
    has_b, act, res = LINEAR_VARIANTS[variant]
    x, w, b, r, model, pmag, exact, rep = _case(M, K, Nout, pieces, xscale)
    n = 3 * K + 1
    gamma = n * U32 / (1 - n * U32)
    kern = gamma * (pmag + (b.double().abs() if has_b else 0)) + K * 2.0 ** -126
    out = {}
    for name, pre, pre_tol in (("model", model, kern), ("float64", exact, kern + rep)):
        pre = pre + b.double() if has_b else pre
        want, tol = ACTS[act](pre), LIPSCHITZ[act] * pre_tol
        act_dev = 0.0
        if act != "none":
            act_dev = float((ACTS[act](pre.float()).double() - want).abs().max())
            tol = tol + 4 * act_dev
        if res:
            want = want + r.double()
            tol = tol + U32 * want.abs()
        out[name] = (want.numpy(), tol.numpy(), act_dev)
    args = (pieces, x, w, b if has_b else None, r if res else None, M, K, Nout, act, res == "in place")
    y1 = _linear(*args)
    y2 = _linear(*args)
    got = y1[:, 8:8 + Nout]
    assert not np.isnan(got).any()                                           # every output written, nothing outside X[M, K] read
    assert np.isnan(np.delete(y1, np.s_[8:8 + Nout], axis=-1)).all()         # channels outside the output slice untouched
    assert y1.tobytes() == y2.tobytes()                                      # a second launch: the same bytes
    few = min(M, 5)
    assert _linear(*args, rows=few).tobytes() == y1[:few].tobytes()          # the first rows alone: the same bytes
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(M))     # a row's bytes do not depend on its place
    pargs = (pieces, x[perm], w, args[3], r[perm] if res else None) + args[5:]
    assert _linear(*pargs)[:, 8:8 + Nout].tobytes() == np.ascontiguousarray(got[perm.numpy()]).tobytes()
    line = f"ssr_linear_split {pieces} {M}x{K}x{Nout} {variant} x * {xscale:g}:"
    errs = {}
    for name, (want, tol, act_dev) in out.items():
        errs[name] = np.abs(got.astype(np.float64) - want)
        line += f" vs {name} max |err| {errs[name].max():.3e}, max err / bound {np.max(errs[name] / tol):.3f};"
    print(line + f" fp32 CPU activation deviation {out['model'][2]:.3e}")
    for name, (want, tol, _) in out.items():
        assert (errs[name] <= tol).all(), (name, float(errs[name].max()), float(np.max(errs[name] / tol)))


@pytest.mark.parametrize("variant", list(LINEAR_VARIANTS))
@pytest.mark.parametrize("pieces", PIECES)
@pytest.mark.parametrize("case", SHAPES, ids=IDS)
def test_linear_split_matches_the_piece_model_and_float64(case, pieces, variant):
    _check(case, pieces, variant)


@pytest.mark.parametrize("pieces,xscale", [("f16", 2.0 ** -16), ("f16", 7.5e3), ("bf16", 1e-7)],
                         ids=["f16 x 2^-16 (the subnormal lo piece is the whole error)", "f16 x 7.5e3 (the top of fp16)", "bf16 dY 1e-7"])
@pytest.mark.parametrize("case", SHAPES, ids=IDS)
def test_linear_split_value_regimes(case, pieces, xscale):
    for variant in ("plain", "bias"):
        _check(case, pieces, variant, xscale)


@pytest.mark.parametrize("variant", ["plain", "bias+gelu_tanh+res", "bias+res in place"])
@pytest.mark.parametrize("pieces", PIECES)
def test_linear_split_on_the_128_tile(pieces, variant):
    """16 x 16 = 256 tiles of 128 x 128 is where the launcher leaves the 64 x 64 tile (none of SHAPES gets there): masked in M and
    Nout, K = 72 = two steps of 32 and a quarter of a third.  The first-rows check of _check then compares the two tile shapes bit
    for bit."""
    _check((1930, 72, 1924), pieces, variant)


def test_pack_layout_and_two_packs_give_the_same_bytes():
    """the header's layout: entry [n][kg] = 8 hi pieces then 8 lo pieces of W[n][8 kg .. 8 kg + 7], zeros past K, fp16 pieces of 2^10 W"""
    from satlas_super_resolution_amd import hip
    from satlas_super_resolution_amd.linear_split import pack_split_weight, split_pieces
    for (_, K, Nout) in SHAPES:
        w = torch.randn(Nout, K, generator=torch.Generator().manual_seed(K)) / K ** 0.5
        wd = w.cuda()
        for pieces, dt, scale in (("f16", torch.float16, 1024.0), ("bf16", torch.bfloat16, 1.0)):
            a, b = pack_split_weight(wd, _code(pieces)), pack_split_weight(wd, _code(pieces))
            KG = (K + 7) // 8
            assert a.numel() == hip.lib().ssr_linear_split_pack_bytes(Nout, K) == 32 * Nout * KG
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
            hi, lo = split_pieces(w * scale, pieces)
            want = torch.zeros(Nout, KG, 2, 8, dtype=dt)
            pad = torch.zeros(Nout, KG * 8, 2, dtype=torch.float64)
            pad[:, :K, 0], pad[:, :K, 1] = hi, lo
            want[:] = pad.reshape(Nout, KG, 8, 2).permute(0, 1, 3, 2).to(dt)
            assert a.cpu().view(torch.int16).numpy().tobytes() == want.view(torch.int16).numpy().tobytes()


def test_linear_split_error_codes():
    from satlas_super_resolution_amd import hip
    from satlas_super_resolution_amd.linear_split import pack_split_weight
    L = hip.lib()
    x = torch.zeros(8, 16, device="cuda")
    w = torch.zeros(8, 16, device="cuda")
    wpk = pack_split_weight(w, hip.SPLIT_F16)
    y = torch.full((8, 8), 7.0, device="cuda")

    def call(xv=hip.view(x), wp=wpk.data_ptr(), rv=hip.NULL_VIEW, yv=hip.view(y), pieces=hip.SPLIT_F16, M=8, K=16, Nout=8, act=0, bias=None):
        return L.ssr_linear_split(xv, wp, bias, rv, yv, pieces, M, K, Nout, act, hip.stream_ptr())

    assert call(K=6) == -2 and call(Nout=6) == -2 and call(M=(1 << 22) + 1) == -2 and call(Nout=(1 << 22) + 4, yv=hip.View(y.data_ptr(), (1 << 22) + 4, 0)) == -2
    assert call(xv=hip.NULL_VIEW) == -1 and call(yv=hip.NULL_VIEW) == -1 and call(wp=None) == -1
    assert call(M=0) == -1 and call(K=0) == -1 and call(Nout=0) == -1 and call(act=4) == -1 and call(act=-1) == -1
    assert call(pieces=0) == -1 and call(pieces=3) == -1 and call(pieces=hip.F32 + 100) == -1
    assert call(xv=hip.View(x.data_ptr(), 16, 4)) == -1 and call(yv=hip.View(y.data_ptr(), 8, 4)) == -1       # view narrower than its channels
    assert call(xv=hip.View(x.data_ptr() + 4, 16, 0)) == -1 and call(wp=wpk.data_ptr() + 4) == -1              # misaligned
    assert call(bias=y.data_ptr() + 2) == -1
    assert call(rv=hip.View(y.data_ptr(), 8, 4)) == -1 and call(yv=hip.View(y.data_ptr(), 6, 0), Nout=4) == -1
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                                            # no launch in any of these cases
    # the pack entry: the same codes, against a sentinel-filled output
    out = torch.full((wpk.numel(),), 7, dtype=torch.uint8, device="cuda")

    def pack(wp=w.data_ptr(), Nout=8, K=16, pieces=hip.SPLIT_BF16, op=out.data_ptr()):
        return L.ssr_linear_split_pack(wp, Nout, K, pieces, op, hip.stream_ptr())

    assert pack(wp=None) == -1 and pack(op=None) == -1 and pack(Nout=0) == -1 and pack(K=0) == -1 and pack(pieces=0) == -1 and pack(pieces=7) == -1
    assert pack(wp=w.data_ptr() + 4) == -1 and pack(op=out.data_ptr() + 8) == -1
    assert pack(K=6) == -2 and pack(Nout=6) == -2
    assert L.ssr_linear_split_pack_bytes(0, 16) < 0 and L.ssr_linear_split_pack_bytes(8, 0) < 0 and L.ssr_linear_split_pack_bytes(8, 20) == 8 * 3 * 32
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    assert call() == 0 and pack() == 0
    torch.cuda.synchronize()
    assert bool((y == 0.0).all()) and bool((out == 0).all())
