"""Differentiable LPIPS without a GPU: the new C symbols are declared, exported and bound; LPIPS.forward_with_grad refuses what it
does not cover before anything is launched; and the inputs of the GPU gradient tests are fit for the purpose (a finite fp64
reference gradient, no all-zero tap pixel of the reconstruction, where torch autograd and the kernel's definition part)."""
import os
import re

import pytest
import torch

import lpips_backward_ref as R
from util import ROOT

NEW_SYMBOLS = ("vt_lpips_tap_backward", "vt_relu_backward", "vt_lpips_prep_backward")


@pytest.fixture(scope="module")
def model():
    from vidtok_amd.lpips import LPIPS

    m = LPIPS(pretrained=False)
    m.load_state_dict(R.state_dict(), strict=True)
    return m.eval()


def _pair(shape=(2, 3, 32, 32)):
    g = torch.Generator().manual_seed(0)
    return torch.rand(shape, generator=g) * 2 - 1, (torch.rand(shape, generator=g) * 2 - 1).requires_grad_(True)


def test_new_symbols_declared_exported_bound(built_lib):
    from vidtok_amd import lib, ops

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vidtok_amd.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in include/vidtok_amd.h"
        assert hasattr(built_lib, name) and name in lib.SIGNATURES
        assert getattr(built_lib, name).argtypes == lib.SIGNATURES[name][1]
    for fn in ("lpips_tap_backward", "relu_backward", "lpips_prep_backward"):
        assert callable(getattr(ops, fn))


def test_kernel_arguments_checked_without_gpu(built_lib):
    from vidtok_amd import lib

    # pointers are never dereferenced: validation fails first
    assert built_lib.vt_lpips_tap_backward(16, 16, 16, None, -1, 16, lib.VT_F16, 1, 4, 4, 64, None) == -1 and b"fp32 or bf16" in built_lib.vt_last_error()
    assert built_lib.vt_lpips_tap_backward(16, 16, 16, None, -1, 16, lib.VT_BF16, 1, 4, 4, 96, None) == -1 and b"C=96" in built_lib.vt_last_error()
    assert built_lib.vt_lpips_tap_backward(16, 16, 16, 8, lib.VT_BF16, 16, lib.VT_BF16, 1, 4, 4, 64, None) == -1 and b"aligned" in built_lib.vt_last_error()
    assert built_lib.vt_relu_backward(16, lib.VT_F32, 16, 16, lib.VT_BF16, 12, None) == -1 and b"multiple of 8" in built_lib.vt_last_error()
    assert built_lib.vt_relu_backward(16, lib.VT_BF16, 16, 16, lib.VT_F32, 16, None) == -1 and b"dy_dtype" in built_lib.vt_last_error()
    assert built_lib.vt_lpips_prep_backward(16, lib.VT_F16, 16, 16, 1, 16, 16, None) == -1 and b"VT_BF16" in built_lib.vt_last_error()
    assert built_lib.vt_lpips_prep_backward(None, lib.VT_F32, 16, 16, 1, 16, 16, None) == -1 and b"null" in built_lib.vt_last_error()


def test_forward_with_grad_refusals(built_lib, model):
    from vidtok_amd import lib

    assert callable(model.forward_with_grad)
    x, y = _pair()
    model.set_compute_dtype(torch.float16)
    try:
        with pytest.raises(NotImplementedError, match="float32 or bfloat16"):
            model.forward_with_grad(x, y)
    finally:
        model.set_compute_dtype(torch.float32)
    with torch.autocast("cpu", dtype=torch.float16):                   # the region of the tensors' device decides, as in forward
        with pytest.raises(NotImplementedError, match="float32 or bfloat16"):
            model.forward_with_grad(x, y)
    with pytest.raises(NotImplementedError, match="ground truth"):
        model.forward_with_grad(x.clone().requires_grad_(True), y)
    x5, y5 = _pair((1, 3, 2, 32, 32))
    with pytest.raises(NotImplementedError, match="NCHW"):
        model.forward_with_grad(x5, y5)
    with pytest.raises(lib.VtError, match="no CPU fallback"):
        model.forward_with_grad(x, y)
    with pytest.raises(lib.VtError, match="no CPU fallback"):
        model.forward_with_grad(x, y.detach())                            # ... also where no gradient is asked for
    assert model._packs == {}                                             # nothing was packed, nothing launched


@pytest.mark.parametrize("case", R.GRAD_CASES, ids=[c["name"] for c in R.GRAD_CASES])
def test_gradient_test_inputs_are_fit(case):
    g = R.ref_grad(case["name"])
    assert g.shape == tuple(case["shape"]) and bool(torch.isfinite(g).all()) and g.abs().max() > 0
    assert R.zero_pixels_per_tap(case) == [0, 0, 0, 0, 0]
