"""GPU: csrc/attention.hip through the C ABI (ssr_self_attention_fwd / _bwd, ssr_relu_bwd) against the float64 statement of
satlas_super_resolution_amd/osm_reference.py.

Shapes: C in {128, 256} (the two blocks of the network), token grids 2x2 .. 8x8 (N = 4 .. 64: every supported token count, among them
the (64, 128) and (16, 256) the network produces for a 32 x 32 crop and the largest LDS footprint (64, 256)), Bo in {1, 3}.
Bound: forward and every backward output within 1e-4 * max|reference| - the project's gate for fp32 kernel families; the kernel is
fp32 FMA chains of at most C + 1 terms, whose rounding is ~1e-6 of the largest element.  dbk is zero in exact arithmetic (a constant
added to every key shifts a softmax row uniformly): it is held to 1e-4 * max|dWk| in absolute terms, never relatively.
The inputs are scaled so that the softmax is neither flat nor saturated: the mean over queries of the largest probability lies in
[0.1, 0.9], asserted on every case."""
import ctypes as C

import pytest
import torch

import osm_disc_fixture as fx

pytestmark = pytest.mark.gpu

SENT = 0x7FC5A5A5
GRIDS = [(2, 2), (2, 4), (4, 4), (4, 8), (8, 8)]
GRADS = ("dwq", "dbq", "dwk", "dbk", "dwv", "dbv", "dgamma")


def _hip():
    from satlas_super_resolution_amd import hip
    return hip, hip.lib()


def _ref():
    from satlas_super_resolution_amd import osm_reference
    return osm_reference


class Run:
    """device buffers and descriptor of one attention problem; x / y / dy / dx are channel slices [coff, coff + C) of [Bo, N, cs] buffers"""

    def __init__(self, x, dy, p, cs=None, coff=0, relu_mask=0, fill=None):
        hip, L = _hip()
        self.hip, self.L = hip, L
        Bo, N, Cc = x.shape
        cs = cs or Cc
        self.shape, self.cs, self.coff = (Bo, N, Cc), cs, coff

        def wide(t=None):
            b = torch.zeros(Bo, N, cs, dtype=torch.float32, device="cuda")
            if fill is not None:
                b.view(torch.int32).fill_(fill)
            if t is not None:
                b[..., coff:coff + Cc] = t.float().cuda()
            return b
        self.x, self.y, self.dy, self.dx = wide(x), wide(), wide(dy), wide()
        self.p = {k: v.float().contiguous().cuda() for k, v in p.items()}
        self.g = {k: torch.zeros_like(self.p[k[1:]]) for k in GRADS}
        self.save = torch.zeros(Bo * int(L.ssr_self_attention_save_floats(N, Cc)), dtype=torch.float32, device="cuda")
        self.scratch = torch.zeros(int(L.ssr_self_attention_scratch_floats(Bo, N, Cc)), dtype=torch.float32, device="cuda")
        d = hip.AttnDesc()
        d.Bo, d.N, d.C = Bo, N, Cc
        v = lambda t: hip.View(t.data_ptr(), cs, coff)
        d.x, d.y, d.dy, d.dx, d.relu_mask = v(self.x), v(self.y), v(self.dy), v(self.dx), relu_mask
        for k in ("wq", "bq", "wk", "bk", "wv", "bv", "gamma"):
            setattr(d, k, self.p[k].data_ptr())
        for k in GRADS:
            setattr(d, k, self.g[k].data_ptr())
        d.save, d.scratch = self.save.data_ptr(), self.scratch.data_ptr()
        self.d = d

    def fwd(self):
        self.hip.check(self.L.ssr_self_attention_fwd(C.byref(self.d), self.hip.stream_ptr()), "ssr_self_attention_fwd")
        torch.cuda.synchronize()
        return self.y[..., self.coff:self.coff + self.shape[2]].cpu()

    def bwd(self, zero=True):
        if zero:
            for t in self.g.values():
                t.zero_()
        self.hip.check(self.L.ssr_self_attention_bwd(C.byref(self.d), self.hip.stream_ptr()), "ssr_self_attention_bwd")
        torch.cuda.synchronize()
        out = {k: t.cpu() for k, t in self.g.items()}
        out["dx"] = self.dx[..., self.coff:self.coff + self.shape[2]].cpu()
        return out


def reference(x, dy, p):
    R = _ref()
    y, s = R.attention_forward(x, p)
    return y, s, R.attention_backward(dy, x, p, s)


def close(got, ref, what):
    err = float((got.double().reshape(ref.shape) - ref).abs().max())
    bound = 1e-4 * float(ref.abs().max())
    print(f"{what}: max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("Bo", [1, 3])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("Cc", [128, 256])
def test_forward_and_backward_match_float64(Cc, grid, Bo):
    N = grid[0] * grid[1]
    x, dy, p = fx.attention_case(1000 * Cc + 10 * N + Bo, Bo, N, Cc, gamma=0.6 if Bo == 1 else -0.8)
    y, s, g = reference(x, dy, p)
    peak = float(s["a"].max(dim=2).values.mean())
    assert 0.1 <= peak <= 0.9, peak
    r = Run(x, dy, p)
    close(r.fwd(), y, "y")
    got = r.bwd()
    for k in ("dx", "dwq", "dbq", "dwk", "dwv", "dbv", "dgamma"):
        close(got[k], g[k], k)
    dbk = float(got["dbk"].abs().max())
    print(f"dbk: max |.| {dbk:.3e}, bound {1e-4 * float(g['dwk'].abs().max()):.3e}")
    assert dbk <= 1e-4 * float(g["dwk"].abs().max())
    # two runs give the same bytes, and the parameter gradients are ADDED to
    r2 = Run(x, dy, p)
    y2 = r2.fwd()
    got2 = r2.bwd()
    assert torch.equal(y2.view(torch.int32), r.fwd().view(torch.int32))
    for k, t in got.items():
        assert torch.equal(t.view(torch.int32), got2[k].view(torch.int32)), k
    twice = r2.bwd(zero=False)
    for k in GRADS:
        assert torch.equal(twice[k], got[k] + got[k]), k


def test_relu_mask_and_a_frozen_discriminator():
    """relu_mask: dx is multiplied by (x > 0); without gradient pointers only dx is produced"""
    hip, L = _hip()
    x, dy, p = fx.attention_case(7, 2, 16, 256)
    x = torch.relu(x)                                    # the input of the block is a ReLU's output in the network
    y, s, g = reference(x, dy, p)
    r = Run(x, dy, p, relu_mask=1)
    close(r.fwd(), y, "y")
    got = r.bwd()
    close(got["dx"], g["dx"] * (x > 0), "dx masked")
    assert float((x > 0).double().mean()) < 0.75 and bool((got["dx"][x <= 0] == 0).all())
    for k in GRADS:
        setattr(r.d, k, None)
    for t in r.g.values():
        t.fill_(3.0)
    r.dx.zero_()
    frozen = r.bwd(zero=False)
    assert torch.equal(frozen["dx"], got["dx"])
    assert all(bool((t == 3.0).all()) for k, t in frozen.items() if k != "dx")


@pytest.mark.parametrize("N,Cc", [(64, 128), (16, 256)])
def test_gamma_zero_is_the_identity_bit_for_bit(N, Cc):
    x, dy, p = fx.attention_case(11 + N, 2, N, Cc, gamma=0.0)
    r = Run(x, dy, p)
    assert torch.equal(r.fwd().view(torch.int32), x.float().view(torch.int32))
    got = r.bwd()                                        # q / k / v receive no gradient, x receives dy
    assert torch.equal(got["dx"].view(torch.int32), dy.float().view(torch.int32))
    for k in ("dwq", "dbq", "dwk", "dbk", "dwv", "dbv"):
        assert not bool(got[k].any()), k
    assert bool(got["dgamma"].abs() > 0)


@pytest.mark.parametrize("N,Cc", [(64, 128), (8, 256)])
def test_a_channel_slice_of_a_wider_buffer_touches_nothing_else(N, Cc):
    x, dy, p = fx.attention_case(23 + N, 3, N, Cc)
    y, s, g = reference(x, dy, p)
    r = Run(x, dy, p, cs=Cc + 24, coff=8, fill=SENT)
    close(r.fwd(), y, "y in a slice")
    got = r.bwd()
    close(got["dx"], g["dx"], "dx in a slice")
    for buf in (r.y, r.dx):
        b = buf.view(torch.int32).cpu()
        assert bool((b[..., :8] == SENT).all()) and bool((b[..., 8 + Cc:] == SENT).all())
    tight = Run(x, dy, p)
    assert torch.equal(tight.fwd().view(torch.int32), r.fwd().view(torch.int32))      # the same bytes as in a tight buffer


def test_relu_bwd_masks_by_the_output():
    hip, L = _hip()
    gen = torch.Generator().manual_seed(5)
    y = torch.relu(torch.randn(37, 8, generator=gen)).cuda()
    g = torch.randn(37, 8, generator=gen).cuda()
    dst = torch.full((37, 8), 9.0, device="cuda")
    v = lambda t: hip.View(t.data_ptr(), 8, 0)
    hip.check(L.ssr_relu_bwd(v(g), v(y), v(dst), 37, 1, hip.stream_ptr()), "ssr_relu_bwd")
    torch.cuda.synchronize()
    assert torch.equal(dst[:, 0], torch.where(y[:, 0] > 0, g[:, 0], torch.zeros_like(g[:, 0]))) and bool((dst[:, 1:] == 9.0).all())
    hip.check(L.ssr_relu_bwd(hip.View(g.data_ptr(), 8, 2), hip.View(y.data_ptr(), 8, 2), hip.View(dst.data_ptr(), 8, 2), 37, 5, hip.stream_ptr()),
              "ssr_relu_bwd")
    torch.cuda.synchronize()
    assert torch.equal(dst[:, 2:7], torch.where(y[:, 2:7] > 0, g[:, 2:7], torch.zeros_like(g[:, 2:7]))) and bool((dst[:, 7] == 9.0).all())
