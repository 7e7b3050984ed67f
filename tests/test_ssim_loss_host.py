"""CPU: the SSIM loss of train.ssim_opt as stated in satlas_super_resolution_amd/ssim_loss.py (what csrc/ssim.hip computes) - the
window and edge cases, the closed-form gradient against autograd in float64, the transposed-filter weight rule the kernel gathers
with, and the option handling of train_config_from_opt."""
import copy
import json
import os

import pytest
import torch

from conftest import GOLDEN
from satlas_super_resolution_amd import ssim_loss as SL

SHAPES = [(3, 3), (3, 4), (4, 5), (5, 7), (9, 6), (37, 53)]      # one-sided and two-sided folds of the padding, and a plain size


def _pair(h, w, seed, n=2, c=3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, c, h, w, generator=g, dtype=torch.float64), torch.rand(n, c, h, w, generator=g, dtype=torch.float64)


def test_window_values():
    g = SL.window()
    assert g.dtype == torch.float64 and abs(float(g.sum()) - 1.0) < 1e-15
    want = torch.tensor([0.12008, 0.23388, 0.29208, 0.23388, 0.12008], dtype=torch.float64)
    assert float((g - want).abs().max()) < 5e-6
    assert torch.equal(g, g.flip(0))


def test_constant_images_have_the_closed_form_ssim():
    for a, b in ((0.3, 0.8), (0.0, 1.0), (1.0, 1.0), (0.0, 0.0)):
        x, y = torch.full((1, 2, 6, 7), a, dtype=torch.float64), torch.full((1, 2, 6, 7), b, dtype=torch.float64)
        s = SL.ssim_map(x, y)
        want = (2 * a * b + SL.C1) / (a * a + b * b + SL.C1) * SL.C2 / (SL.C2 + 1e-12 / (a * a + b * b + SL.C1))
        # D = B1 B2 + eps with B2 = C2 exactly:  S = A1 C2 / (B1 C2 + eps)
        assert float((s - want).abs().max()) <= 1e-12, (a, b)
        near = (2 * a * b + SL.C1) / (a * a + b * b + SL.C1) * SL.C2 / (SL.C2 + 1e-12)
        assert abs(want - near) <= 1.2e-5       # the issue's form, exact where B1 = 1; eps / (C1 C2) = 1.1e-5 at most otherwise
        assert abs(float(SL.ssim_loss_reference(x, y, 0.5)) - 0.5 * min(max((1 - want) / 2, 0.0), 1.0)) <= 1e-12


def test_equal_images_give_zero_loss_and_gradient():
    x, y = _pair(9, 11, seed=1)
    # S = N / (N + eps) with N = B1 B2 >= C1 C2: (1 - S) / 2 <= eps / (2 C1 C2) = 5.6e-6 whatever the image, far less on noise
    loss, grad = SL.ssim_loss_grad_reference(x, x.clone(), 1.0)
    assert 0.0 <= float(loss) <= 1e-12 / (2 * SL.C1 * SL.C2)
    assert float(loss) < 1e-9                                         # uniform noise: N ~ 1e-2
    _, g_xy = SL.ssim_loss_grad_reference(x, y, 1.0)
    assert float(grad.abs().max()) <= 1e-6 * float(g_xy.abs().max())
    xa = x.clone().requires_grad_(True)
    SL.ssim_loss_reference(xa, x.clone(), 1.0).backward()
    assert float(xa.grad.abs().max()) <= 1e-6 * float(g_xy.abs().max())


def test_loss_is_unchanged_by_flips_and_transposes():
    x, y = _pair(7, 10, seed=2)
    base = float(SL.ssim_loss_reference(x, y, 0.1))
    for f in (lambda t: t.flip(-1), lambda t: t.flip(-2), lambda t: t.transpose(-1, -2).contiguous(), lambda t: t.flip(-1).transpose(-1, -2).contiguous()):
        assert abs(float(SL.ssim_loss_reference(f(x), f(y), 0.1)) - base) <= 1e-14


@pytest.mark.parametrize("h,w", SHAPES)
def test_closed_form_gradient_equals_autograd_in_float64(h, w):
    x, y = _pair(h, w, seed=h * 100 + w)
    # a part where the clamp's lower side is met (x == y), a flat part and an anticorrelated part
    y[0, 0] = x[0, 0]
    y[1, 1] = 1.0 - x[1, 1]
    xa = x.clone().requires_grad_(True)
    loss = SL.ssim_loss_reference(xa, y, 0.1)
    loss.backward()
    l2, g2 = SL.ssim_loss_grad_reference(x, y, 0.1)
    assert abs(float(loss.detach()) - float(l2)) <= 1e-14
    assert float((g2 - xa.grad).abs().max()) <= 1e-12 * float(xa.grad.abs().max())


def _kernel_ft_weight(p, q, n, g):
    """csrc/ssim.hip ft_weight, restated: the taps of F's row q that land on p directly or folded from the padding"""
    if q < 0 or q >= n:
        return 0.0
    w = 0.0
    t = p - q
    if -2 <= t <= 2:
        w += g[t + 2]
    if 1 <= p <= 2:
        t = -p - q
        if t >= -2:
            w += g[t + 2]
    if n - 3 <= p <= n - 2:
        t = 2 * (n - 1) - p - q
        if t <= 2:
            w += g[t + 2]
    return w


@pytest.mark.parametrize("n", [3, 4, 5, 6, 7, 12])
def test_gather_weights_are_the_transposed_fold_matrix(n):
    m = SL.fold_matrix(n)
    g = SL.window().tolist()
    assert float((m.sum(1) - 1).abs().max()) < 1e-15                  # every row of F sums to one
    for p in range(n):
        for q in range(-2, n + 2):
            want = float(m[q, p]) if 0 <= q < n else 0.0
            assert abs(_kernel_ft_weight(p, q, n, g) - want) < 1e-15, (n, p, q)
            if abs(p - q) > 2 and 0 <= q < n:
                assert want == 0.0                                    # Ft reaches no further than two pixels
    if n >= 5:
        assert float(m[:, 0].sum()) == pytest.approx(g[2] + g[3] + g[4])   # row 0 receives no folded tap
    # reflect-padded filtering is NOT the transpose
    assert not torch.allclose(m, m.t())


def _opts():
    return json.load(open(os.path.join(GOLDEN, "ssr_options.json")))


def test_train_config_from_opt_reads_the_shipped_ssimloss_file():
    from satlas_super_resolution_amd.models.ssr_esrgan_model import step_config_from_opt, train_config_from_opt
    opts = _opts()
    opt = opts["ssimloss_esrgan_s2naip_urban.yml"]
    before = copy.deepcopy(opt)
    cfg = train_config_from_opt(opt)
    assert opt == before                                              # the caller's dictionary is left as it was
    assert cfg.ssim == {"loss_weight": 0.1}
    urban = step_config_from_opt(opts["esrgan_s2naip_urban.yml"])
    assert urban.ssim is None
    urban.ssim = {"loss_weight": 0.1}
    assert cfg == urban
    with pytest.raises(NotImplementedError, match="ssim_opt"):        # the older function still refuses (tests/test_host_boundary.py)
        step_config_from_opt(opt)


def test_train_config_from_opt_equals_step_config_for_the_files_that_ran_before():
    from satlas_super_resolution_amd.models.ssr_esrgan_model import step_config_from_opt, train_config_from_opt
    opts = _opts()
    for name in ("allbands_esrgan_s2naip_urban.yml", "esrgan_s2naip_full.yml", "esrgan_s2naip_urban.yml", "old-naip_esrgan_s2naip_urban.yml",
                 "rand_crop_esrgan_s2naip_urban.yml", "infer_example.yml", "infer_grid_example.yml"):
        a, b = train_config_from_opt(opts[name]), step_config_from_opt(opts[name])
        assert a == b and a.ssim is None, name
    with pytest.raises(NotImplementedError, match="clip_opt"):
        train_config_from_opt(opts["cliploss_esrgan_s2naip_urban.yml"])


def test_train_config_from_opt_refuses_other_types_and_keys_by_name():
    from satlas_super_resolution_amd.models.ssr_esrgan_model import train_config_from_opt
    opt = _opts()["ssimloss_esrgan_s2naip_urban.yml"]
    o = copy.deepcopy(opt)
    o["train"]["ssim_opt"]["type"] = "Other"
    with pytest.raises(NotImplementedError, match=r"ssim_opt\.type.*Other"):
        train_config_from_opt(o)
    o = copy.deepcopy(opt)
    o["train"]["ssim_opt"]["window_size"] = 11
    with pytest.raises(NotImplementedError, match=r"ssim_opt\.window_size"):
        train_config_from_opt(o)
    o = copy.deepcopy(opt)
    del o["train"]["ssim_opt"]["loss_weight"]
    assert train_config_from_opt(o).ssim == {"loss_weight": 1.0}


def test_step_config_carries_the_term_and_the_abi_names_the_kernel():
    from satlas_super_resolution_amd import hip
    from satlas_super_resolution_amd.train_step import N_LOSS, StepConfig
    assert StepConfig().ssim is None and N_LOSS == 9
    assert "ssr_ssim_loss" in hip.ABI_SYMBOLS
