"""Generates the OSMObjDiscriminator fixtures under tests/golden/ by EXECUTING the reference's own class on the CPU.

    python tools/make_osm_disc_golden.py      # needs the reference checkout (oracle/ref_shim.py: SSR_REFERENCE_ROOT)

Runs on a build machine only; no test, smoke() or benchmark imports it.  The reference's module ssr/archs/osm_obj_discriminator_arch.py
imports only torch and the registry, so it loads under oracle.ref_shim's stand-ins as they are.

The network is num_in_ch = 27, num_feat = 8.  The object branch's weights are filled by the rule of tests/osm_disc_fixture.py (exact in
float32, stable across library versions: the top 24 bits of numpy's PCG64 raw stream), not stored - they are 3 MB; the small U-Net half
is stored as the reference's class initialised it, weight_u / weight_v after ten training forwards (a checkpoint's have seen many
power iterations; the initial random ones give a sigma near zero and logits of 1e7).  No case may have an o_out that is identically
zero.  Files, every one below the 1 MiB limit of a committed file:

  osm_disc_head.pt             kwargs, the 50 key names and shapes in the reference's order, seed, the U-Net half's tensors, x [2, 27, 16, 16],
                               weight_u / weight_v after one training forward
  osm_disc_case0.pt            osm_objs [5, 3, 32, 32], the loss weights w (mixed sign), out / o_out of the evaluation forward and of the
                               training forward in float32 and float64, the attention and ReLU statistics, the float32-to-float64 distances
  osm_disc_case0_grads_*.pt    for the loss sum(o_out * w) + mean(out) of the training forward: every parameter gradient and both input
                               gradients, in float32 and in float64, in pieces
  osm_disc_case1.pt, case2.pt  osm_objs [3, 3, 16, 32] and [1, 3, 16, 16]: the evaluation outputs only

A seed is kept only if the conditions of tests/osm_disc_fixture.py hold (branch alive, attention neither uniform nor one-hot, every float32
gradient of the reference within 1e-4 * max|float64 gradient|): no test rests on a ReLU decision that float32 cannot make.
key_conv.bias has a gradient that is zero in exact arithmetic (a constant added to every key shifts each softmax row uniformly); it is
excluded from the relative gate and recorded as it came out.
"""
from __future__ import annotations

import importlib
import os
import sys
from collections import OrderedDict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import osm_disc_fixture as fx  # noqa: E402
from oracle import ref_shim  # noqa: E402
from satlas_super_resolution_amd import osm_reference  # noqa: E402

CASES = ((5, 32, 32), (3, 16, 32), (1, 16, 16))
FILE_BYTES = 1_000_000
POWER_ITERATIONS = 10


def load_class():
    ref_shim.load_reference_archs()
    return importlib.import_module("ssr.archs.osm_obj_discriminator_arch").OSMObjDiscriminator


def build(cls, sd, dtype):
    net = cls(**fx.KWARGS)
    net.load_state_dict(sd, strict=True)
    return net.to(dtype)


def run(cls, sd, x, osm, w, dtype, train):
    net = build(cls, sd, dtype)
    net.train(train)
    xx, oo = x.to(dtype).detach().clone().requires_grad_(train), osm.to(dtype).detach().clone().requires_grad_(train)
    if not train:
        with torch.no_grad():
            out, o_out = net(xx, oo)
        return dict(out=out, o_out=o_out)
    out, o_out = net(xx, oo)
    loss = (o_out * w.to(dtype)).sum() + out.mean()
    loss.backward()
    grads = OrderedDict((n, p.grad.detach().clone()) for n, p in net.named_parameters())
    grads["x"], grads["osm_objs"] = xx.grad.detach().clone(), oo.grad.detach().clone()
    uv = OrderedDict((k, v.detach().clone()) for k, v in net.state_dict().items() if k.endswith(("weight_u", "weight_v")))
    return dict(out=out.detach(), o_out=o_out.detach(), grads=grads, uv=uv)


def stats(sd, osms):
    """fx.branch_stats of a list of crops batches, pooled (a 16 x 16 crop has ONE o_out element: a share needs the pool)"""
    return fx.branch_stats({k: v.double() for k, v in sd.items()}, [o.double() for o in osms])


def main():
    cls = load_class()
    for seed in range(32):
        torch.manual_seed(seed)
        net = cls(**fx.KWARGS)
        g = torch.Generator().manual_seed(4000 + seed)
        x = torch.rand(2, 27, 16, 16, generator=g)
        osms = [torch.rand(bo, 3, h, w, generator=g) for bo, h, w in CASES]
        wts = torch.randn(5, 1, 2, 2, generator=g)
        with torch.no_grad():          # trained-like: weight_u / weight_v of a checkpoint have seen many power iterations
            net.train()
            for _ in range(POWER_ITERATIONS):
                net(x, osms[0])
        sd = OrderedDict((k, v.detach().clone()) for k, v in net.state_dict().items())
        keys = [(k, tuple(v.shape)) for k, v in sd.items()]
        assert keys[:len(fx.OBJ_KEYS)] == fx.OBJ_KEYS and keys[len(fx.OBJ_KEYS):] == fx.unet_keys(fx.KWARGS["num_feat"], fx.KWARGS["num_in_ch"]), \
            "the reference's state_dict is not the recorded key list"
        unet_state = OrderedDict((k, v) for k, v in sd.items() if not k.startswith("o_"))
        sd.update(fx.object_branch_state(seed))
        assert (wts > 0).any() and (wts < 0).any()
        st = [stats(sd, osms), stats(sd, osms[:1])]          # all cases pooled; the gradient case alone
        each = [stats(sd, [o])["alive"] for o in osms]       # and no case whose o_out is identically zero
        print(f"seed {seed}: {st} {each}")
        if not all(fx.stats_ok(s) for s in st) or min(each) == 0.0:
            continue
        r32 = run(cls, sd, x, osms[0], wts, torch.float32, True)
        r64 = run(cls, sd, x, osms[0], wts, torch.float64, True)
        dist, worst = OrderedDict(), 0.0
        for n, g64 in r64["grads"].items():
            d = float((r32["grads"][n].double() - g64).abs().max() / g64.abs().max().clamp_min(1e-300))
            dist[n] = d
            if not n.endswith("key_conv.bias"):
                worst = max(worst, d)
        for n in ("out", "o_out"):
            dist[n] = float((r32[n].double() - r64[n]).abs().max() / r64[n].abs().max())
        print(f"seed {seed}: worst float32-to-float64 gradient distance {worst:.2e}; outputs {dist['out']:.2e} {dist['o_out']:.2e}")
        for a in ("o_attention1", "o_attention2"):
            kb, kw = r64["grads"][f"{a}.key_conv.bias"], r64["grads"][f"{a}.key_conv.weight"]
            assert float(kb.abs().max()) <= 1e-9 * float(kw.abs().max()), "key_conv.bias gradient is not zero in float64"
        if worst <= fx.GRAD_GATE:
            break
    else:
        raise SystemExit("no seed meets the conditions")

    head = dict(arch="OSMObjDiscriminator", kwargs=fx.KWARGS, keys=keys, seed=seed, unet_state=unet_state, x=x,
                uv_after=r32["uv"], uv_after_f64=r64["uv"], grad_names=list(r64["grads"].keys()),
                input_shapes={"x": tuple(x.shape), "osm_objs": tuple(osms[0].shape)},
                n_object_parameters=sum(int(torch.tensor(s).prod()) for _, s in fx.OBJ_KEYS),
                rule="tests/osm_disc_fixture.py: object_branch_state(seed)", grad_gate=fx.GRAD_GATE)
    torch.save(head, os.path.join(fx.GOLDEN, "osm_disc_head.pt"))
    for ci, osm in enumerate(osms):
        e32 = run(cls, sd, x, osm, None, torch.float32, False)
        e64 = run(cls, sd, x, osm, None, torch.float64, False)
        case = dict(osm_objs=osm, eval_out=e32["out"], eval_o_out=e32["o_out"], eval_out_f64=e64["out"], eval_o_out_f64=e64["o_out"])
        if ci == 0:
            case.update(w=wts, train_out=r32["out"], train_o_out=r32["o_out"], train_out_f64=r64["out"], train_o_out_f64=r64["o_out"],
                        f32_to_f64=dist, key_conv_bias_grad_is_zero=True, stats_pooled=st[0], stats_case0=st[1])
        torch.save(case, os.path.join(fx.GOLDEN, f"osm_disc_case{ci}.pt"))
    for f in os.listdir(fx.GOLDEN):
        if f.startswith("osm_disc_case0_grads_"):
            os.remove(os.path.join(fx.GOLDEN, f))
    cur, size, nfile = {}, 0, 0

    def flush():
        nonlocal cur, size, nfile
        if cur:
            torch.save(cur, os.path.join(fx.GOLDEN, f"osm_disc_case0_grads_{nfile:02d}.pt"))
            cur, size, nfile = {}, 0, nfile + 1

    for tag, res in (("f32", r32), ("f64", r64)):
        for name, gr in res["grads"].items():
            for j, piece in enumerate(fx.pieces(gr.flatten())):
                nbytes = piece.numel() * piece.element_size()
                if size + nbytes > FILE_BYTES:
                    flush()
                cur[(tag, name, j)] = piece
                size += nbytes
    flush()
    total = 0
    for f in sorted(os.listdir(fx.GOLDEN)):
        if f.startswith("osm_disc_"):
            n = os.path.getsize(os.path.join(fx.GOLDEN, f))
            assert n < 1 << 20, f
            total += n
            print(f, n)
    print("total", total)


if __name__ == "__main__":
    main()
