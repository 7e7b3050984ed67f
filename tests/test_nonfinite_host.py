"""CPU: the entry points and host plumbing of the non-finite guard (csrc/finite.hip, ssr_quantize_u8_checked) - argument checks that
return SSR_EINVAL without a launch, the ctypes table, and the host branch of the inference quantiser refusing NaN / Inf."""
import ctypes as C

import numpy as np
import pytest
import torch


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from satlas_super_resolution_amd import hip
    return hip, hip.lib()


def test_new_entry_points_are_exported_and_reject_bad_arguments_without_a_launch():
    hip, L = _lib()
    for s in ("ssr_nonfinite_scan", "ssr_adam_step_guarded", "ssr_quantize_u8_checked"):
        assert s in hip.ABI_SYMBOLS and hasattr(L, s)
    assert L.ssr_abi_version() == 3
    one = lambda t, v: (t * 1)(v)
    fake = 1 << 20                      # a 16-byte aligned address that is never dereferenced: every call below fails its checks first
    src, n = one(C.c_void_p, fake), one(C.c_int64, 16)
    assert L.ssr_nonfinite_scan(src, n, 1, None, None) == -1                              # NULL flag
    assert L.ssr_nonfinite_scan(src, one(C.c_int64, -1), 1, fake, None) == -1            # n < 0
    assert L.ssr_nonfinite_scan(src, n, 0, fake, None) == -1                              # no range
    assert L.ssr_nonfinite_scan(src, n, hip.SCAN_MAX_RANGES + 1, fake, None) == -1        # more ranges than the kernel takes
    assert L.ssr_nonfinite_scan(one(C.c_void_p, fake + 2), n, 1, fake, None) == -1       # not a float address
    assert L.ssr_nonfinite_scan(one(C.c_void_p, None), n, 1, fake, None) == -1           # NULL range of n > 0
    assert L.ssr_adam_step_guarded(None, fake, fake, None) == -1
    a = hip.AdamArgs(fake, fake, fake, fake, None, 16, fake, fake, 0.9, 0.99, 1e-8, 0.0, 1.0)
    assert L.ssr_adam_step_guarded(C.byref(a), None, fake, None) == -1                   # NULL flag
    assert L.ssr_adam_step_guarded(C.byref(a), fake, None, None) == -1                   # NULL skip counter
    a.n = 0
    assert L.ssr_adam_step_guarded(C.byref(a), fake, fake, None) == -1
    assert L.ssr_quantize_u8_checked(fake, fake, 1, 3, 4, 4, 1, None, None) == -1         # NULL counter
    assert L.ssr_quantize_u8_checked(fake, fake, 1, 3, 4, 4, 2, fake, None) == -1         # bad mode


def test_host_quantiser_raises_on_non_finite_outputs_and_names_the_exact_mode():
    from satlas_super_resolution_amd.utils import infer_utils as U
    y = torch.tensor([[[[-0.2, 0.5, 254.9 / 255, 1.7]]]]).repeat(1, 3, 1, 1)
    assert U.quantize_output(y, "fp32h")[0, 0, :, 0].tolist() == [0, 127, 254, 255]     # finite: unchanged
    for bad in (float("nan"), float("inf"), float("-inf")):
        z = y.clone()
        z[0, 1, 0, 2] = bad
        with pytest.raises(FloatingPointError, match="fp32f") as e:
            U.quantize_output(z, "fp32h")
        assert "1 non-finite" in str(e.value) and "fp32h" in str(e.value)
    z = y.clone()
    z[0, :, 0, 0] = float("nan")
    with pytest.raises(FloatingPointError, match="3 non-finite output sample") as e:
        U.quantize_output(z, "fp32")
    assert "fp32f" not in str(e.value)              # the advice belongs to the fp16-split mode only


def test_checked_buffer_layout_round_trips_on_the_host():
    from satlas_super_resolution_amd.metrics import split_checked
    shape = (2, 3, 5, 3)                             # 90 bytes: the counter starts at byte 92
    buf = torch.zeros(96, dtype=torch.uint8)
    buf[:90] = torch.arange(90, dtype=torch.uint8)
    buf[92:96].view(torch.int32)[0] = 7
    img, bad = split_checked(buf, shape)
    assert bad == 7 and tuple(img.shape) == shape and np.array_equal(img.numpy().reshape(-1), np.arange(90))
