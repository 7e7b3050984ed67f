"""Shared by the OSMObjDiscriminator tests and tools/make_osm_disc_golden.py: the rule that fills the object branch's weights, and the
loader of tests/golden/osm_disc_*.pt.  (Not a test module.)

The object branch has fixed widths: 765,859 parameters, 3 MB - o_conv3.weight alone is 2 MB, above the size limit of a committed file.
Its weights are therefore not stored but FILLED BY A RULE that is exact in float32 and does not depend on a library version:

    tensor number t of OBJ_KEYS (n elements, fan_in f):
        r    = numpy.random.PCG64(1000 * seed + t).random_raw(n)          the generator's raw 64-bit stream
        k    = r >> 40                                                    its top 24 bits: an integer below 2^24
        u    = float32(k) * 2^-24                                         exact
        w    = (2 u - 1) * float32(s / sqrt(f))                           2u - 1 is exact; ONE float32 rounding
    s = 3 for the weights of o_conv1..4 and value_conv (trained-like: three times the bound of torch's default initialisation), 2 for
    query_conv / key_conv (the energies carry the product of the two), 1 for biases;
    o_conv4.bias = 0.05, o_attention1.gamma = 0.7, o_attention2.gamma = -0.4.

With the default initialisation the fixtures would test nothing: gamma = 0 switches attention off and zeroes the gradients of q / k / v,
and the final ReLU leaves o_out identically zero.  The generator asserts, and tests/test_osm_disc_host.py asserts again on what it
loads: the share of o_out elements > 0 lies in [0.25, 0.75]; the mean over queries of the largest attention probability lies in
[0.1, 0.9] for both blocks - both over the three cases pooled (the 16 x 16 case has a single o_out element) and over the gradient case
alone; every float32 gradient of the reference is within 1e-4 * max|float64 gradient| of the float64 one.
"""
import glob
import math
import os
from collections import OrderedDict

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KWARGS = dict(num_in_ch=27, num_feat=8, skip_connection=True)
GAMMAS = {"o_attention1.gamma": 0.7, "o_attention2.gamma": -0.4}
O_CONV4_BIAS = 0.05
W_SCALE, QK_SCALE, B_SCALE = 3.0, 2.0, 1.0
ALIVE_RANGE, PEAK_RANGE, GRAD_GATE = (0.25, 0.75), (0.1, 0.9), 1e-4
PIECE = 120_000                      # elements per stored piece of a gradient: 960 KB in float64, below the 1 MiB limit of a committed file


def _obj_keys():
    keys = []
    conv = lambda n, co, ci, k: keys.extend([(n + ".weight", (co, ci, k, k)), (n + ".bias", (co,))])

    def attention(n, c):
        keys.append((n + ".gamma", (1,)))
        conv(n + ".query_conv", c // 8, c, 1)
        conv(n + ".key_conv", c // 8, c, 1)
        conv(n + ".value_conv", c, c, 1)
    conv("o_conv1", 64, 3, 4)
    conv("o_conv2", 128, 64, 4)
    attention("o_attention1", 128)
    conv("o_conv3", 256, 128, 4)
    attention("o_attention2", 256)
    conv("o_conv4", 1, 256, 4)
    return keys


OBJ_KEYS = _obj_keys()               # the reference's first 26 state_dict keys, in its order


def unet_keys(num_feat=8, num_in_ch=27):
    nf = num_feat
    keys = [("conv0.weight", (nf, num_in_ch, 3, 3)), ("conv0.bias", (nf,))]
    for i, (co, ci, k) in enumerate(((2 * nf, nf, 4), (4 * nf, 2 * nf, 4), (8 * nf, 4 * nf, 4), (4 * nf, 8 * nf, 3), (2 * nf, 4 * nf, 3),
                                     (nf, 2 * nf, 3), (nf, nf, 3), (nf, nf, 3)), start=1):
        keys += [(f"conv{i}.weight_orig", (co, ci, k, k)), (f"conv{i}.weight_u", (co,)), (f"conv{i}.weight_v", (ci * k * k,))]
    return keys + [("conv9.weight", (1, nf, 3, 3)), ("conv9.bias", (1,))]


def rule_tensor(seed: int, t: int, shape, scale: float) -> torch.Tensor:
    n = math.prod(shape)
    k = np.random.PCG64(1000 * seed + t).random_raw(n) >> np.uint64(40)
    u = k.astype(np.float32) * np.float32(2.0 ** -24)
    w = (np.float32(2.0) * u - np.float32(1.0)) * np.float32(scale)
    assert w.dtype == np.float32
    return torch.from_numpy(w).reshape(shape)


def object_branch_state(seed: int) -> "OrderedDict[str, torch.Tensor]":
    sd = OrderedDict()
    for t, (key, shape) in enumerate(OBJ_KEYS):
        if key in GAMMAS:
            sd[key] = torch.full((1,), GAMMAS[key], dtype=torch.float32)
        elif key == "o_conv4.bias":
            sd[key] = torch.full((1,), O_CONV4_BIAS, dtype=torch.float32)
        else:
            wkey = key.rsplit(".", 1)[0] + ".weight"
            wshape = dict(OBJ_KEYS)[wkey]
            fan_in = wshape[1] * wshape[2] * wshape[3]
            s = ((QK_SCALE if ("query_conv" in key or "key_conv" in key) else W_SCALE) if key.endswith(".weight") else B_SCALE) / math.sqrt(fan_in)
            sd[key] = rule_tensor(seed, t, shape, float(np.float32(s)))
    return sd


def branch_stats(sd, osms):
    """pooled over a list of osm_objs batches: the share of o_out elements > 0, and per attention block the mean over all queries of
    the largest probability of a row (a 16 x 16 crop has ONE o_out element: a share needs the pool)"""
    from satlas_super_resolution_amd import osm_reference
    alive, p1, p2 = [], [], []
    for osm in osms:
        o_out, (a1, a2) = osm_reference.object_branch(sd, osm, return_attention=True)
        alive.append((o_out.detach() > 0).flatten().double())
        p1.append(a1.max(dim=2).values.flatten().double())
        p2.append(a2.max(dim=2).values.flatten().double())
    return dict(alive=float(torch.cat(alive).mean()), peak1=float(torch.cat(p1).mean()), peak2=float(torch.cat(p2).mean()))


def stats_ok(s) -> bool:
    return (ALIVE_RANGE[0] <= s["alive"] <= ALIVE_RANGE[1] and PEAK_RANGE[0] <= s["peak1"] <= PEAK_RANGE[1]
            and PEAK_RANGE[0] <= s["peak2"] <= PEAK_RANGE[1])


def attention_case(seed: int, B: int, N: int, Cc: int, gamma: float = 0.6):
    """float64 inputs of one SelfAttentionBlock in token form: (x [B, N, C], dy, p).  The projections are scaled so that the energies
    have a standard deviation of about 1.5 whatever C is: the softmax is then neither flat nor saturated (asserted by the callers)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    dk = Cc // 8
    s = math.sqrt(1.5 / (math.sqrt(dk) * Cc))
    p = dict(wq=rnd(dk, Cc) * s, bq=rnd(dk) * 0.1, wk=rnd(dk, Cc) * s, bk=rnd(dk) * 0.1, wv=rnd(Cc, Cc) / math.sqrt(Cc), bv=rnd(Cc) * 0.1,
             gamma=torch.tensor([gamma], dtype=torch.float64))
    return rnd(B, N, Cc), rnd(B, N, Cc), p


def pieces(flat: torch.Tensor):
    return [flat[i:i + PIECE].clone() for i in range(0, flat.numel(), PIECE)]


def load_head():
    return torch.load(os.path.join(GOLDEN, "osm_disc_head.pt"), weights_only=False)


def full_state(head=None) -> "OrderedDict[str, torch.Tensor]":
    """the checkpoint the reference's class saved: the ruled object branch, then the stored U-Net half"""
    head = head or load_head()
    sd = object_branch_state(head["seed"])
    sd.update(head["unet_state"])
    return sd


def load_case(i: int):
    return torch.load(os.path.join(GOLDEN, f"osm_disc_case{i}.pt"), weights_only=False)


def load_grads():
    """{'f32' | 'f64': {name: gradient}} of case 0, reassembled from the piece files"""
    head = load_head()
    shapes = dict(OBJ_KEYS + unet_keys(KWARGS["num_feat"], KWARGS["num_in_ch"]))
    shapes.update(head["input_shapes"])
    parts = {}
    for f in sorted(glob.glob(os.path.join(GOLDEN, "osm_disc_case0_grads_*.pt"))):
        for (tag, name, j), t in torch.load(f, weights_only=False).items():
            parts.setdefault((tag, name), {})[j] = t
    out = {"f32": OrderedDict(), "f64": OrderedDict()}
    for name in head["grad_names"]:
        for tag in ("f32", "f64"):
            p = parts[(tag, name)]
            out[tag][name] = torch.cat([p[j] for j in range(len(p))]).reshape(shapes[name])
    return out
