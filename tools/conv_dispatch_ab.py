"""sha256 of what ssr_conv2d writes for one small descriptor per (kernel family, dtype), and of one ssr_conv2d_batch call of the four 2x2
parity-class descriptors of a 4x4 stride-2 dgrad in bf16 and in fp32x3.  Two builds of the library launch the same kernels with the
same arguments exactly when their transcripts are equal line for line (profiles/conv_dispatch/).

  python tools/conv_dispatch_ab.py --out transcript.txt          # needs the GPU

The descriptors are the ones tests/test_gpu_conv_dispatch.py runs: find_case() asks ssr_conv2d_variant (no launch) for the smallest
N = 1 layer of a fixed candidate order that the library sends to the family by itself.
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_conv_dispatch_golden as sweep  # noqa: E402

# the candidate lists of csrc/conv.hip, in their order: family -> (last digit of ssr_conv2d_variant, ssr_conv2d_impl code that forces it)
FAMILY = {"thin": (7, 5), "ws": (8, 1), "big": (9, 4), "bigx3": (9, 4), "x3r": (5, 7), "x3q": (6, 6), "res": (1, None), "pipelined": (None, 3)}
ORDER = {"fp32h": ["thin", "bigx3", "x3r", "pipelined"],
         "fp32x3": ["thin", "bigx3", "x3r", "x3q", "pipelined"],
         "fp32": ["thin", "x3r", "res", "pipelined"],
         "bf16": ["thin", "ws", "big", "res", "pipelined"]}
FWD_CODE = {"fp32": 0, "bf16": 1, "fp32x3": 2, "fp32h": 3}
# candidates, smallest first: the grid, then the generator body's 64 -> 32 layer before the other channel counts, then the nearest-x2 read
GRIDS = [32, 64, 128, 256, 512]
CHANNELS = [(64, 32), (8, 32), (64, 3), (96, 64), (64, 64)]


def find_case(hip, mode, family):
    """(Cin, Cout, grid, up) of the first candidate the library sends to `family` by itself, or None (the ring kernel: the register-tiled
    one takes every layer it could run)."""
    digit = FAMILY[family][0]
    for grid in GRIDS:
        for cin, cout in CHANNELS:
            for up in (1, 2):
                d = sweep.make_desc(hip, FWD_CODE[mode], 3, 1, cin, cout, grid, 1, hip.ACT_NONE, "up" if up == 2 else "")
                w = hip.lib().ssr_conv2d_variant(C.byref(d)) % 10
                if w == digit or (digit is None and w in (2, 4)):
                    return cin, cout, grid, up
    return None


def cases(hip):
    for mode, order in ORDER.items():
        for family in order:
            c = find_case(hip, mode, family)
            if c is not None:
                yield mode, family, c


class Layer:
    """One 3x3 layer with seeded weights and input; run(impl) launches it and returns the output tensor."""

    def __init__(self, mode, cin, cout, grid, up):
        import torch
        from satlas_super_resolution_amd import engine, hip
        self.hip, self.engine, self.up, self.hi = hip, engine, up, grid // up
        g = torch.Generator().manual_seed(1000 * grid + 10 * cin + cout)
        self.st = engine.ParamStore([engine.ConvSpec("c", cout, cin, 3, 1, True, False)], hip.dtype_code(mode))
        self.st.load_state_dict({"c.weight": torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / (cin * 9) ** 0.5),
                                 "c.bias": torch.randn(cout, generator=g) * 0.1})
        self.st.pack()
        tdt = torch.bfloat16 if mode == "bf16" else torch.float32
        self.x = (torch.randn(1, self.hi, self.hi, cin, generator=g) * 0.5).to(tdt).cuda().contiguous()
        self.y = torch.zeros(1, grid, grid, engine.rup(cout, 8), dtype=tdt, device="cuda")
        self.cb = engine._ConvBuilder(self.st, 1)
        self.d = self.cb.conv(engine.Launcher(), "c", hip.view(self.x), self.hi, self.hi, hip.view(self.y), up=up, cin=cin)

    def run(self, impl):
        """None when the forced family cannot run the layer (SSR_EUNSUP)"""
        import torch
        self.y.zero_()
        rc = self.hip.lib().ssr_conv2d_impl(C.byref(self.d), self.hip.stream_ptr(), impl)
        if rc == -2:
            return None
        self.hip.check(rc, f"impl {impl}")
        torch.cuda.synchronize()
        return self.y.clone()


def parity_class_batch(mode):
    """dgrad of a 4x4 stride-2 layer, 64 <- 128 channels on a 32 x 32 grid, B = 2: four 2x2 descriptors through ssr_conv2d_batch"""
    import torch
    from satlas_super_resolution_amd import engine, hip
    cout, cin, gh, B = 128, 64, 32, 2
    g = torch.Generator().manual_seed(7)
    st = engine.ParamStore([engine.ConvSpec("c", cout, cin, 4, 2, True, False)], hip.dtype_code(mode))
    st.load_state_dict({"c.weight": torch.randn(cout, cin, 4, 4, generator=g) * (1.0 / (cin * 16) ** 0.5), "c.bias": torch.zeros(cout)})
    st.pack()
    tdt = torch.bfloat16 if mode == "bf16" else torch.float32
    dy = (torch.randn(B, gh, gh, cout, generator=g) * 0.5).to(tdt).cuda().contiguous()
    y = torch.zeros(B, 2 * gh, 2 * gh, cin, dtype=tdt, device="cuda")
    L = engine.Launcher()
    cb = engine._ConvBuilder(st, B)
    cb.dgrad(L, "c", hip.view(dy), gh, gh, hip.view(y))
    _, args, _ = L.calls[0]
    hip.check(hip.lib().ssr_conv2d_batch(args[0], args[1], hip.stream_ptr()), "batch")
    torch.cuda.synchronize()
    return y


def digest(t):
    return hashlib.sha256(t.contiguous().view(-1).view(__import__("torch").uint8).cpu().numpy().tobytes()).hexdigest()


def transcript():
    from satlas_super_resolution_amd import hip
    lines = []
    for mode, family, (cin, cout, grid, up) in cases(hip):
        lines.append(f"{mode} {family} {cin}->{cout} {grid}x{grid} up{up} {digest(Layer(mode, cin, cout, grid, up).run(0))}")
    for mode in ("bf16", "fp32x3"):
        lines.append(f"{mode} batch4 128->64 32x32 {digest(parity_class_batch(mode))}")
    return lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    out = transcript()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))
