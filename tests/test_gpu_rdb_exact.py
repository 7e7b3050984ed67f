"""GPU: the two fused ResidualDenseBlock kernels - csrc/rdb_fwd.hip (8 x 8 tiles) and csrc/rdb_tile.hip (8 x 16 tiles) - each forced through
ssr_rdb_desc.tile and held, one at a time, to the float64 restatement of the descriptor contract in tests/rdb_lattice.py.  Never kernel
against kernel: a mistake in what the two share (the 5-pixel halo recomputed per tile, zero outside the image written into the LDS slices,
the chunk, tap and k-substep order) shows here.

  exact        one stage (forward 1..5) or slice (backward 4..0) at a time on lattice operands, every stage up to it by torch.equal
  teacher      normal weights and inputs, the engine's scales: every stored stage against float64 from the device's own inputs of it
  memory       the engine's aliasing forms and the fully separated form give the same bytes; channel-sliced views; NaN wherever nothing
               may be read; sentinels around every output view; inputs unchanged; w_next changes nothing; refusals write nothing

The weights are packed by the project's own packing (ParamStore.pack, add_repack, add_rdb_gather), the launches go through the C ABI with
hand-built descriptors.  Shapes: the smallest at which tiling can go wrong (rdb_lattice.SHAPES), N = 1 and 3."""
import pytest
import torch

import rdb_lattice as rl

pytestmark = pytest.mark.gpu


def _id(nhw):
    return "x".join(map(str, nhw))


# ================================================================================================ exact
@pytest.mark.parametrize("tile", rl.TILES)
@pytest.mark.parametrize("nhw", rl.NHW, ids=_id)
@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_exact_stages(direction, nhw, tile):
    """every stage under test in turn; the buffers carry NaN wherever nothing may be read, the engine's aliasing form"""
    msgs = []
    for case in (c for c in rl.EXACT_CASES if c.direction == direction and (c.N, c.H, c.W) == nhw):
        ep = rl.EXACT_FWD if direction == "fwd" else rl.EXACT_BWD
        res = rl.run(direction, tile, rl.exact_packed(case), ep, rl.exact_tensors(case))
        assert res.rc == 0, case.name
        msg = rl.exact_mismatch(case, res)
        if msg:
            msgs.append(msg)
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("tile", rl.TILES)
@pytest.mark.parametrize("what,case,mutation", rl.MUTATIONS, ids=[m[0] for m in rl.MUTATIONS])
def test_device_result_rejects_the_mutated_reference(what, case, mutation, tile):
    """the comparison is not empty: what the device stored for the named case equals the contract's bits and differs from the bits of
    the reference with the mistake made in it (tests/test_rdb_lattice_host.py shows the two references differ; this shows which side
    the kernel is on)"""
    ep = rl.EXACT_FWD if case.direction == "fwd" else rl.EXACT_BWD
    res = rl.run(case.direction, tile, rl.exact_packed(case), ep, rl.exact_tensors(case))
    got = res.out if case.k in (0, 5) else res.slices[case.k]
    assert torch.equal(got, rl.exact_expected(case)[0][case.k]), rl.exact_mismatch(case, res)
    assert not torch.equal(got, rl.exact_expected(case, **mutation(case))[0][case.k]), what


# ================================================================================================ teacher-forced
def _teacher_run(nhw, tile, name, **kw):
    ep = rl.TEACHER[name]
    t = rl.teacher_data(*nhw)
    r2 = t["r2"] if ep["r2"] else None
    fwd = rl.run("fwd", tile, rl.packed("teacher", a5=ep["alpha5"]), ep, dict(x=t["x"], r2=r2), **kw)
    masks = torch.cat([fwd.slices[j] for j in range(1, 5)], 1)
    bwd = rl.run("bwd", tile, rl.packed("teacher", a5=ep["alpha5"]), ep, dict(d_out=t["d_out"], r2=t["d_r2"] if ep["r2"] else None, masks=masks), **kw)
    return t, ep, fwd, bwd


@pytest.mark.parametrize("tile", rl.TILES)
@pytest.mark.parametrize("name", list(rl.TEACHER))
@pytest.mark.parametrize("nhw", rl.NHW, ids=_id)
def test_teacher_forced_stages(nhw, name, tile):
    """forward, then the backward with the forward's stored slices as masks (the engine's form); prints every figure before it asserts"""
    t, ep, fwd, bwd = _teacher_run(nhw, tile, name)
    assert fwd.rc == 0 and bwd.rc == 0
    res = {f"x{k}": v for k, v in rl.teacher_forward_check(t["x"], t["r2"], ep, fwd.slices, fwd.out).items()}
    res.update({f"d{j}": v for j, v in rl.teacher_backward_check(t["d_out"], t["d_r2"], ep, fwd.slices, bwd.slices, bwd.out).items()})
    for k, (ok, st) in res.items():
        print(f"teacher {_id(nhw)} {name} tile {tile} {k}: differing {st['differing']} of {st['numel']}, worst {st['ulps']:.3f} ulp, mean {st['mean']:.2e}")
    bad = {k: st for k, (ok, st) in res.items() if not ok}
    assert not bad, bad
    assert fwd.guards_ok and fwd.inputs_ok and bwd.guards_ok and bwd.inputs_ok


# ================================================================================================ memory contract
MEM_SHAPES = [(3, 3, 5), (1, 9, 17)]              # a sub-tile and a ragged shape


def _same(a, b):
    return torch.equal(a.slice_bits, b.slice_bits) and torch.equal(a.out_bits, b.out_bits)


@pytest.mark.parametrize("tile", rl.TILES)
@pytest.mark.parametrize("nhw", MEM_SHAPES, ids=_id)
def test_aliasing_views_poison_sentinels_and_prefetch(nhw, tile):
    """base: the engine's form (forward in == slices, backward out == slices with mask the forward buffer), cs = 192, no poison.  Every
    other form - poisoned, channel-sliced in the aliased and in the fully separated form, with w_next set - gives the same bytes,
    finite, leaves every sentinel and every input alone."""
    t, ep, f0, b0 = _teacher_run(nhw, tile, "rrdb", poison=False)
    assert f0.rc == 0 and b0.rc == 0 and f0.guards_ok and f0.inputs_ok and b0.guards_ok and b0.inputs_ok
    masks = torch.cat([f0.slices[j] for j in range(1, 5)], 1)
    pk = rl.packed("teacher", a5=ep["alpha5"])
    tens = {"fwd": dict(x=t["x"], r2=t["r2"]), "bwd": dict(d_out=t["d_out"], r2=t["d_r2"], masks=masks)}
    base = {"fwd": f0, "bwd": b0}
    for direction in ("fwd", "bwd"):
        forms = [("poisoned", dict(poison=True)), ("w_next", dict(poison=True, w_next=True))]
        forms += [(f"sliced {'aliased' if lay.alias else 'separated'}{' poisoned' if p else ''}", dict(layout=lay, poison=p))
                  for lay in rl.SLICED[direction] for p in (False, True)]
        forms.append(("separated", dict(layout=rl.Layout(alias=False), poison=True)))
        for what, kw in forms:
            r = rl.run(direction, tile, pk, ep, tens[direction], **kw)
            assert r.rc == 0, (direction, what)
            assert bool(torch.isfinite(r.out).all()) and all(bool(torch.isfinite(s).all()) for s in r.slices.values()), (direction, what)
            assert _same(r, base[direction]), f"{direction} {what}: other bytes than the engine's form"
            assert r.guards_ok, f"{direction} {what}: a sentinel outside the output views changed"
            assert r.inputs_ok, f"{direction} {what}: an input changed"


@pytest.mark.parametrize("tile", rl.TILES)
def test_refusals_write_nothing(tile):
    from satlas_super_resolution_amd import hip
    nhw = (1, 3, 5)
    t = rl.teacher_data(*nhw)
    ep = rl.TEACHER["rrdb"]
    pk = rl.packed("teacher", a5=ep["alpha5"])
    tens = {"fwd": dict(x=t["x"], r2=t["r2"]), "bwd": dict(d_out=t["d_out"], r2=t["d_r2"], masks=torch.cat([t["x"], t["r2"]], 1))}

    def setter(path, value):
        def tweak(d):
            obj = d
            for p in path[:-1]:
                obj = getattr(obj, p)
            if isinstance(path[-1], int):
                obj[path[-1]] = value
            else:
                setattr(obj, path[-1], value)
        return tweak

    def shifted(view, field, by):
        return lambda d: setattr(getattr(d, view), field, getattr(getattr(d, view), field) + by)

    EINVAL, EUNSUP = -1, -2
    both = [("fp32 dtype", setter(("dtype",), hip.F32), EUNSUP), ("fp32x3 dtype", setter(("dtype",), hip.F32X3), EUNSUP),
            ("NULL in", setter(("inp", "p"), None), EINVAL), ("NULL slices", setter(("slices", "p"), None), EINVAL),
            ("NULL out", setter(("out", "p"), None), EINVAL),
            ("in.cs % 8", shifted("inp", "cs", 4), EINVAL), ("in.coff % 8", shifted("inp", "coff", 4), EINVAL),
            ("slices.cs % 8", shifted("slices", "cs", 4), EINVAL), ("slices.coff % 8", shifted("slices", "coff", 4), EINVAL),
            ("out.cs % 8", shifted("out", "cs", 4), EINVAL), ("out.coff % 8", shifted("out", "coff", 4), EINVAL),
            ("r2.cs % 4", shifted("r2", "cs", 2), EINVAL), ("r2.coff % 4", shifted("r2", "coff", 2), EINVAL)]
    both += [(f"NULL w[{k}]", setter(("w", k), None), EINVAL) for k in range(5)]
    only_bwd = [("no mask", setter(("mask", "p"), None), EINVAL), ("mask.cs % 4", shifted("mask", "cs", 2), EINVAL),
                ("mask.coff % 4", shifted("mask", "coff", 2), EINVAL)]
    for direction in ("fwd", "bwd"):
        for what, tweak, code in both + (only_bwd if direction == "bwd" else []):
            r = rl.run(direction, tile, pk, ep, tens[direction], layout=rl.Layout(alias=False), tweak=tweak)
            assert r.rc == code, f"{direction} {what}: returned {r.rc}, not {code}"
            assert r.untouched, f"{direction} {what}: refused, but wrote"
