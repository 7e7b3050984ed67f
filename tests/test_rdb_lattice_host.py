"""CPU: tests/rdb_lattice.py itself - the float64 stage references against autograd of the plain dense block, the exactness condition of
every committed case, the emulation of max(v, 0.2f v) and of the bf16 store against torch's own conversions, the cap of the teacher-forced
criterion (an fp32 convolution in another summation order meets it on every committed case), and the mutations: each of the mistakes the
exact comparison exists for, made on the reference side, changes the expected bits of a named committed case."""
import pytest
import torch
import torch.nn.functional as F

import rdb_lattice as rl


def test_stage_references_agree_with_autograd_of_the_dense_block():
    """forward64 / backward64 without any rounding against rrdbnet_arch.py:37-44 (+ :68) under autograd, to 1e-12"""
    g = torch.Generator().manual_seed(7)
    N, H, W = 2, 6, 11
    Wt, Bt = rl.teacher_weights()
    Wd, Bd = {j: w.double() for j, w in Wt.items()}, {j: b.double() for j, b in Bt.items()}
    ep = rl.TEACHER["rrdb"]
    a5, b1, b2 = (float(torch.tensor(ep[n], dtype=torch.float32)) for n in ("alpha5", "beta1", "beta2"))
    x = torch.randn(N, rl.NF, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    r2, d_out, d_r2 = (torch.randn(N, rl.NF, H, W, generator=g, dtype=torch.float64) for _ in range(3))
    feats, pres = [x], {}
    for k in range(1, 5):
        pres[k] = F.conv2d(torch.cat(feats, 1), Wd[k], Bd[k], padding=1)
        pres[k].retain_grad()
        feats.append(F.leaky_relu(pres[k], rl.SLOPE))
    out = a5 * F.conv2d(torch.cat(feats, 1), Wd[5], Bd[5], padding=1) + b1 * x + b2 * r2
    out.backward(d_out)
    same = lambda a, b: float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())      # noqa: E731
    ref = rl.forward64(x.detach(), Wd, Bd, ep, r2, round_=lambda v: v)
    for k in range(1, 5):
        assert same(ref[k][0], feats[k].detach()), f"x{k}"
    assert same(ref[5][0], out.detach())
    masks = {k: feats[k].detach() for k in range(1, 5)}
    Wf = dict(Wd)
    Wf[5] = Wd[5] * a5
    back = rl.backward64(d_out, masks, Wf, ep, d_r2, round_=lambda v: v)
    for k in range(1, 5):
        assert same(back[k][0], pres[k].grad), f"dpre{k}"
    assert same(back[0][0], x.grad + b2 * d_r2)


def test_exactness_condition_of_every_case():
    """sum |terms| < 2^24 quanta, the handed-over stages positive bf16 lattice values (asserted inside exact_expected), every stage
    under test with outputs of both signs; prints the largest margin"""
    worst = max(rl.EXACT_CASES, key=lambda c: rl.exact_expected(c)[1])
    for c in rl.EXACT_CASES:
        want, margin = rl.exact_expected(c)
        assert margin < 1.0, c.name
        if c.H * c.W >= 15:
            assert bool((want[c.k] > 0).any()) and bool((want[c.k] < 0).any()), f"{c.name}: one-sided outputs"
    print(f"largest margin: {worst.name}: {rl.exact_expected(worst)[1]:.5f} of 2^24 quanta")
    assert len({(c.N, c.H, c.W) for c in rl.EXACT_CASES}) == 13
    for n in (1, 3):                              # both epilogues on a sub-tile and on a ragged shape, at either batch size
        assert {rl.has_r2(n, 3, 5), rl.has_r2(3 if n == 1 else 1, 3, 5)} == {True, False}
        assert {rl.has_r2(n, 9, 17), rl.has_r2(3 if n == 1 else 1, 9, 17)} == {True, False}


def test_planted_mask_values_are_there():
    for c in rl.EXACT_CASES:
        if c.direction == "bwd" and c.k > 0:
            d = rl.exact_data(c)
            bits = d["masks"][c.k].view(torch.int16)
            for n in range(c.N):
                for s in rl.SPECIAL_BITS:
                    assert bool((bits[n] == s).any()), (c.name, s)
            for j in range(c.k + 1, 5):
                assert bool((d["masks"][j].double() > 0).all())


def test_emulation_agrees_with_torch_conversions():
    g = torch.Generator().manual_seed(3)
    special = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 9.2e-41, -9.2e-41, 1e-39, -1e-39, 1.1754944e-38, -1.1754944e-38,
                            1.0 + 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 3 * 2.0 ** -8, -(1.0 + 3 * 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -20,
                            5.0 * (1.0 + 2.0 ** -8), -5.0 * (1.0 + 2.0 ** -8), 3.0e38, -3.0e38, 2.0 ** -133, -(2.0 ** -133), 2.0 ** -134,
                            3 * 2.0 ** -134, -3 * 2.0 ** -134], dtype=torch.float32)
    rnd = torch.cat([torch.randn(20000, generator=g) * s for s in (1.0, 1e-3, 1e3, 1e-38, 1e-40)]).float()
    ints = torch.randint(-2 ** 31, 2 ** 31 - 1, (50000,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    v = torch.cat([special, rnd, ints[torch.isfinite(ints)]])
    want = torch.maximum(v, v * torch.tensor(0.2, dtype=torch.float32)).bfloat16()
    got = rl.bf16_rne(rl.lrelu32(v.double()))
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert torch.equal(rl.bf16_rne(v.double()).view(torch.int16), v.bfloat16().view(torch.int16))
    # the mask convention: 1 where m > 0 as a real number - +0, -0 and the negative subnormal take 0.2f, the positive subnormal 1
    m = torch.tensor(rl.SPECIAL_BITS, dtype=torch.int16).view(torch.bfloat16).double()
    assert rl.slope_of(m).tolist() == [False, False, True, False]
    x = torch.tensor([0.0, -0.0, 9.2e-41, -9.2e-41, 1.0, -1.0], dtype=torch.float32)
    xg = x.clone().requires_grad_(True)
    F.leaky_relu(xg, 0.2).backward(torch.ones_like(x))
    assert torch.equal(xg.grad == 1.0, rl.slope_of(x.double()))           # torch's leaky_relu_backward


def _fp32_block(x, r2, ep, d_out, d_r2):
    """the dense block and its backward with fp32 F.conv2d on the packed bf16 weights and a bf16 store after every stage: the same contract
    in another summation order"""
    W, B = rl.teacher_weights()
    Wp, Wg = rl.packed_values(W), rl.packed_values(W, ep["alpha5"])
    f = lambda t: t.float()                       # noqa: E731
    s = torch.tensor(0.2, dtype=torch.float32)
    feats, sl = [f(x)], {}
    for k in range(1, 5):
        pre = F.conv2d(torch.cat(feats, 1), f(Wp[k]), B[k], padding=1)
        feats.append(torch.maximum(pre, pre * s).bfloat16().float())
        sl[k] = feats[-1].double()
    a5, b1, b2 = (torch.tensor(ep[n], dtype=torch.float32) for n in ("alpha5", "beta1", "beta2"))
    out = a5 * F.conv2d(torch.cat(feats, 1), f(Wp[5]), B[5], padding=1) + b1 * f(x)
    out = (out + b2 * f(r2)) if ep["r2"] else out
    dpre = {}
    for j in (4, 3, 2, 1, 0):
        acc = sum(F.conv_transpose2d(f(d_out) if i == 5 else f(dpre[i]), f(Wg[i][:, rl.block(j)]), padding=1) for i in range(j + 1, 6))
        if j > 0:
            dpre[j] = torch.where(sl[j] > 0, acc, acc * s).bfloat16().double()
        else:
            dx = acc + b1 * f(d_out)
            dx = (dx + b2 * f(d_r2)) if ep["r2"] else dx
    return sl, out.bfloat16().double(), dpre, dx.bfloat16().double()


@pytest.mark.parametrize("nhw", rl.NHW, ids=lambda s: "x".join(map(str, s)))
def test_fp32_convolution_meets_the_teacher_forced_criterion(nhw):
    """the cap is a condition: another fp32 summation order stays inside it against float64 on every committed case"""
    for name, ep in rl.TEACHER.items():
        t = rl.teacher_data(*nhw)
        sl, out, dpre, dx = _fp32_block(t["x"], t["r2"], ep, t["d_out"], t["d_r2"])
        res = rl.teacher_forward_check(t["x"], t["r2"], ep, sl, out)
        res.update({f"d{j}": v for j, v in rl.teacher_backward_check(t["d_out"], t["d_r2"], ep, sl, dpre, dx).items()})
        bad = {k: st for k, (ok, st) in res.items() if not ok}
        assert not bad, (name, bad)


def _differs(case, **mutation):
    base, _ = rl.exact_expected(case)
    mutated, _ = rl.exact_expected(case, **mutation)
    return not torch.equal(base[case.k], mutated[case.k])


MUTATIONS = rl.MUTATIONS


@pytest.mark.parametrize("what,case,mutation", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutation_is_caught_by_a_committed_case(what, case, mutation):
    assert case in rl.EXACT_CASES
    assert _differs(case, **mutation(case)), f"{what}: {case.name} does not notice"
    print(f"{what}: caught by {case.name}")


def test_mutations_show_on_every_shape_they_can():
    """how wide each mutation hits: the stages whose expected bits change, over the sub-tile shape 3 x 5"""
    for mut, direction in (("halo_bias", "fwd"), ("b5_outside", "fwd"), ("one_at_plus_zero", "bwd"), ("subnormal_as_negative", "bwd"),
                           ("shift_segment", "bwd")):
        hit = [c.name for c in rl.EXACT_CASES if c.direction == direction and (c.N, c.H, c.W) == (1, 3, 5) and _differs(c, mut=mut)]
        print(f"{mut}: {hit}")
        assert hit
