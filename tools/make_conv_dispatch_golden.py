"""What ssr_conv2d_variant / ssr_conv2d_symbol answer for a broad sweep of descriptors, with and without the off switches.

Uses only the public C ABI (include/ssr_hip.h) through satlas_super_resolution_amd.hip, launches nothing and needs no GPU: x, y, w and
the optional views point into a host buffer that no query dereferences.

  python tools/make_conv_dispatch_golden.py --out tests/golden/conv_dispatch_table.json    # every run, one fresh process per switch
  python tools/make_conv_dispatch_golden.py --one                                          # this process's environment, JSON on stdout
  python tools/make_conv_dispatch_golden.py --time 200000                                  # seconds for that many ssr_conv2d_variant calls

tests/test_conv_dispatch_host.py regenerates the table from the built library and compares it with the committed file.
"""
import argparse
import base64
import ctypes as C
import json
import os
import subprocess
import sys
import time
import zlib
from array import array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# the switches are cached at first use: each run is a process of its own.  "" = nothing set
RUNS = ["", "SSR_X3_REGTILE=0", "SSR_F32_REGTILE=0", "SSR_X3_BIGTILE=0", "SSR_CONV_BIGTILE=0", "SSR_CONV_WS=0", "SSR_CONV_THIN=0",
        "SSR_CONV_THIN_F32=0", "SSR_CONV_S2D=0", "SSR_X3_PIPE=1"]
GEOMS = [(3, 1), (2, 1), (4, 2)]
CINS = [8, 24, 64, 96, 160, 256]
COUTS = [1, 3, 8, 32, 64, 128, 256]
GRIDS = [4, 16, 32, 64, 128]
BATCHES = [1, 4, 16, 32]
EXTRAS = ["r1", "m", "x2", "up", "s2d", "r1+m"]

_host = C.create_string_buffer(1 << 16)
_base = (C.addressof(_host) + 255) & ~255


def _view(hip, slot, cs):
    return hip.View(_base + 4096 * slot, cs, 0)


def make_desc(hip, dtype, K, stride, Cin, Cout, grid, N, act, extra=""):
    """One descriptor of the sweep, or None when `extra` does not apply to the geometry (s2d where ssr_conv2d_s2d_ok refuses)."""
    coutpad = (Cout + 31) // 32 * 32
    up = 2 if "up" in extra else 1
    if up == 2 and (stride != 1 or grid % 2):
        return None
    if "s2d" in extra and not (K == 4 and hip.lib().ssr_conv2d_s2d_ok(dtype, Cin, Cout, coutpad)):
        return None
    hi = grid * stride // up
    ycs = (Cout + 7) // 8 * 8
    d = hip.ConvDesc()
    d.dtype, d.N, d.Hi, d.Wi, d.up, d.Cin = dtype, N, hi, hi, up, Cin
    d.x = _view(hip, 0, Cin)
    d.w, d.CoutPad, d.bias = _base + 4096, coutpad, None
    d.KH = d.KW = K
    d.stride = stride
    d.pad_y = d.pad_x = {3: 1, 2: 0, 4: 1}[K]
    d.Gh = d.Gw = d.Ho = d.Wo = grid
    d.oys = d.oxs = 1
    d.Cout = Cout
    d.y = _view(hip, 2, ycs)
    d.alpha, d.act = 1.0, act
    if "x2" in extra:
        d.x2, d.Cin2 = _view(hip, 3, 32), 32
    if "r1" in extra:
        d.r1, d.r1_nc, d.beta1 = _view(hip, 4, ycs), Cout, 0.2
    if "m" in extra:
        d.m, d.m_c0, d.m_c1 = _view(hip, 5, ycs), 0, Cout
    d.s2d = 1 if "s2d" in extra else 0
    return d


def descriptors(hip):
    """The sweep as (what the descriptor is, descriptor), in a fixed order: every (dtype, geometry, Cin, Cout, grid, N) once plain and
    once with one of EXTRAS, the activation and the extra rotating so that every pairing occurs (about 20 000 descriptors)."""
    k = 0
    for dtype in (hip.F32, hip.BF16, hip.F32X3, hip.F32H3):
        for K, stride in GEOMS:
            for Cin in CINS:
                for Cout in COUTS:
                    for grid in GRIDS:
                        for N in BATCHES:
                            yield (dtype, K, Cin, Cout, grid, N, k % 3, ""), make_desc(hip, dtype, K, stride, Cin, Cout, grid, N, k % 3)
                            for j in range(len(EXTRAS)):          # the first extra, in rotation, that applies here
                                act, extra = (k // 3) % 3, EXTRAS[(k + j) % len(EXTRAS)]
                                d = make_desc(hip, dtype, K, stride, Cin, Cout, grid, N, act, extra)
                                if d is not None:
                                    yield (dtype, K, Cin, Cout, grid, N, act, extra), d
                                    break
                            k += 1


def query(hip, d):
    """'variant|symbol' as the library answers for `d`."""
    lib = hip.lib()
    buf = C.create_string_buffer(160)
    v = lib.ssr_conv2d_variant(C.byref(d))
    rc = lib.ssr_conv2d_symbol(C.byref(d), buf, 160)
    return "%d|%s" % (v, buf.value.decode() if rc == 0 else "rc=%d" % rc)


def sweep():
    """{"rows": the answers, "what": (dtype, K, Cin, Cout, grid, N, act, extra) of each descriptor} in this process's environment"""
    from satlas_super_resolution_amd import hip
    ds = list(descriptors(hip))
    return {"rows": [query(hip, d) for _, d in ds], "what": [w for w, _ in ds]}


def sweep_in_subprocess(setting):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SSR_")}
    if setting:
        name, value = setting.split("=")
        env[name] = value
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one"], env=env, check=True, capture_output=True, text=True).stdout
    return json.loads(out)


def all_runs():
    """{switch setting: sweep() under it}, the runs side by side in fresh processes."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=len(RUNS)) as ex:
        return dict(zip(RUNS, ex.map(sweep_in_subprocess, RUNS)))


def encode(runs):
    """String table + one uint16 index per row (zlib, base64): 10 runs of 20 000 rows stay far below 256 KB."""
    runs = {k: r["rows"] for k, r in runs.items()}
    table = sorted({s for rows in runs.values() for s in rows})
    index = {s: i for i, s in enumerate(table)}
    assert len(table) < 65536
    enc = {k: base64.b64encode(zlib.compress(array("H", [index[s] for s in rows]).tobytes(), 9)).decode() for k, rows in runs.items()}
    return {"strings": table, "rows": len(next(iter(runs.values()))), "byteorder": sys.byteorder, "runs": enc}


def decode(doc):
    out = {}
    for k, b in doc["runs"].items():
        a = array("H")
        a.frombytes(zlib.decompress(base64.b64decode(b)))
        if doc["byteorder"] != sys.byteorder:
            a.byteswap()
        out[k] = [doc["strings"][i] for i in a]
    return out


def time_variant(calls):
    from satlas_super_resolution_amd import hip
    ds = [d for i, (_, d) in enumerate(descriptors(hip)) if i % 101 == 0]
    fn, refs = hip.lib().ssr_conv2d_variant, [C.byref(d) for d in ds]
    fn(refs[0])
    t0 = time.perf_counter()
    for i in range(calls // len(refs) + 1):
        for r in refs:
            fn(r)
    return (time.perf_counter() - t0) * calls / ((calls // len(refs) + 1) * len(refs))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--time", type=int, default=0)
    a = ap.parse_args()
    if a.one:
        json.dump(sweep(), sys.stdout)
    elif a.time:
        print("%.3f s for %d ssr_conv2d_variant calls" % (time_variant(a.time), a.time))
    else:
        doc = encode(all_runs())
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=0)
            f.write("\n")
        print("%d rows x %d runs, %d distinct answers -> %s" % (doc["rows"], len(doc["runs"]), len(doc["strings"]), a.out))
