"""Differentiable LPIPS on the MI355X: the fused tap backward against fp64 autograd of head + max-pool + ReLU mask, the ReLU and prep
backward kernels, the whole gradient against fp64 CPU autograd of the pure-torch restatement (tests/lpips_ref.py), its properties
(value bit-equal to forward, determinism, exact zero on identical images, autocast) and the chain with the decoder's HIP backward.

Gates.  fp32: max|d| / max|ref| <= 1e-5 for the tap kernel (the forward tap test's gate) and <= 1e-4 for the whole pass (the
project's fp32 bound).  bf16 tap kernel: 2^-8 = one rounding of an fp32 value to bf16 (2^-9), doubled.  bf16 whole pass: relative
L2 distance to the fp64 gradient <= 2x the distance of torch's own bf16 autograd of the restatement on the CPU, computed in the test
(the two bf16 paths round at different places)."""
import pytest
import torch

import lpips_backward_ref as R
from lpips_cases import make_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
TAP_GATE = {torch.float32: 1e-5, torch.bfloat16: 2.0 ** -8}


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm()).item()


def frames(v):
    """NCTHW clip -> its frames as NCHW images"""
    return v.permute(0, 2, 1, 3, 4).reshape(-1, v.shape[1], *v.shape[3:])


@pytest.fixture(scope="module")
def model(built_lib):
    from vidtok_amd.lpips import LPIPS

    m = LPIPS(pretrained=False)
    m.load_state_dict(R.state_dict(), strict=True)
    return m.to(DEV).eval()


def _grad(model, x, y, dtype, wts=None):
    """(value, d sum(wts * value) / dy) of forward_with_grad in arithmetic `dtype`"""
    y = y.detach().clone().requires_grad_(True)
    model.set_compute_dtype(dtype)
    try:
        val = model.forward_with_grad(x, y)
        w = torch.ones(val.numel(), device=val.device) if wts is None else wts.to(val.device)
        (val.reshape(-1) * w).sum().backward()
    finally:
        model.set_compute_dtype(torch.float32)
    return val.detach(), y.grad


# ---- 1. vt_lpips_tap_backward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, pool", [(torch.float32, None), (torch.float32, "same"), (torch.bfloat16, None), (torch.bfloat16, "same"),
                                         (torch.bfloat16, "f32")], ids=["f32_nopool", "f32_dpool", "bf16_nopool", "bf16_dpool", "bf16_dpool_f32"])
@pytest.mark.parametrize("C, H, W", [(64, 13, 9), (128, 8, 8), (256, 7, 6), (512, 3, 2), (512, 5, 3)])
def test_tap_backward(built_lib, C, H, W, dtype, pool):
    from vidtok_amd import ops

    g = torch.Generator().manual_seed(C + H * 31 + W)
    N = 3
    feat = torch.relu(torch.randn(2 * N, H, W, C, generator=g)).to(dtype)
    feat[N + 1, 0, 0] = 0.0                                        # an all-zero pixel of f1: the norm term is defined as 0 there
    feat[N, 0, 1, 5] = feat[N, 1, 0, 5] = 7.0                      # two equal maxima in window (0, 0) of frame 0, channel 5
    lw = torch.rand(C, generator=g)
    gout = torch.tensor([0.7, -1.3, 2.1])
    dpool = None
    if pool is not None:
        dpool = torch.randn(N, H // 2, W // 2, C, generator=g).to(dtype if pool == "same" else torch.float32)
        dpool[0, 0, 0, 5] = 3.0
    got = ops.lpips_tap_backward(feat.to(DEV), lw.to(DEV), gout.to(DEV), None if dpool is None else dpool.to(DEV))
    torch.cuda.synchronize()
    want = R.ref_tap_backward(feat, lw, gout, dpool)
    assert got.shape == want.shape and got.dtype == dtype and bool(torch.isfinite(got).all())
    assert bool((got[1, 0, 0] == 0).all())                         # the all-zero pixel: masked, finite
    assert bool((got.cpu()[feat[N:] <= 0] == 0).all())             # the ReLU mask of the tap's convolution
    e = _rel(got, want)
    print(f"[tap backward] C={C} {H}x{W} {dtype} dpool={pool}: max|d|/max|ref| {e:.3e}")
    assert e <= TAP_GATE[dtype], e
    if dpool is not None:                                          # the tie: the pooled gradient goes to (0, 1), the first maximum
        head = ops.lpips_tap_backward(feat.to(DEV), lw.to(DEV), gout.to(DEV), None)
        assert got[0, 1, 0, 5] == head[0, 1, 0, 5]
        assert abs((got[0, 0, 1, 5] - head[0, 0, 1, 5]).item() - 3.0) <= 3.0 * 2.0 ** -7


# ---- 2. vt_relu_backward, vt_lpips_prep_backward --------------------------------------------------------------------------------
@pytest.mark.parametrize("dy_dtype, dtype", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.bfloat16)],
                         ids=["f32", "bf16", "f32_to_bf16"])
def test_relu_backward_bit_equal(built_lib, dy_dtype, dtype):
    from vidtok_amd import ops

    g = torch.Generator().manual_seed(3)
    y = torch.relu(torch.randn(3, 1, 7, 9, 64, generator=g)).to(dtype).to(DEV)       # 1 512 rows of 8: six workgroups
    dy = torch.randn(3, 1, 7, 9, 64, generator=g).to(dy_dtype).to(DEV)
    got = ops.relu_backward(dy, y)
    assert got.dtype == dtype and torch.equal(got, (dy * (y > 0)).to(dtype))
    half = ops.relu_backward(dy[1:], y[1:])                                             # a slice of the saved stack, as the pass reads it
    assert torch.equal(half, got[1:])


@pytest.mark.parametrize("dtype", GRAD_DTYPES, ids=IDS)
def test_prep_backward(built_lib, dtype):
    from vidtok_amd import ops

    g = torch.Generator().manual_seed(4)
    d = torch.randn(3, 17, 19, 8, generator=g).to(dtype)                                # channels 3..7: not read
    scale = torch.tensor([0.458, 0.448, 0.450])
    got = ops.lpips_prep_backward(d.to(DEV), scale.to(DEV))
    want = (d[..., :3].double() / scale.double()).permute(0, 3, 1, 2)
    assert got.shape == (3, 3, 17, 19) and got.dtype == torch.float32 and got.is_contiguous()
    assert _rel(got, want) <= 1e-6


# ---- 3. the whole pass ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", GRAD_DTYPES, ids=IDS)
@pytest.mark.parametrize("case", R.GRAD_CASES, ids=[c["name"] for c in R.GRAD_CASES])
def test_gradient_vs_fp64_autograd(model, case, dtype):
    """Measured on an MI355X (profiles/lpips_backward.md).  fp32, max|d|/max|ref|: 3.2e-6 (p2_32), 3.7e-6 (p3_50x38).  bf16, relative
    L2 ours / torch's bf16 autograd on the CPU: 5.59e-2 / 5.68e-2 (p2_32), 6.48e-2 / 6.64e-2 (p3_50x38)."""
    x, y = make_inputs(case)
    ref = R.ref_grad(case["name"])
    _, got = _grad(model, x.to(DEV), y.to(DEV), dtype, R.pair_weights(x.shape[0]))
    assert got.shape == y.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    if dtype == torch.float32:
        e = _rel(got, ref)
        print(f"[lpips grad] {case['name']} fp32: max|d|/max|ref| {e:.3e} (gate 1e-4)")
        assert e <= 1e-4, e
    else:
        base = R.bf16_grad(case["name"])
        e, eb = _rel_l2(got, ref), _rel_l2(base, ref)
        print(f"[lpips grad] {case['name']} bf16: rel L2 ours {e:.3e}, torch bf16 autograd (CPU) {eb:.3e} (gate 2x = {2 * eb:.3e}); "
              f"max-norm ours {_rel(got, ref):.3e}, torch bf16 {_rel(base, ref):.3e}")
        assert e <= 2 * eb, (e, eb)


# ---- 4. properties --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", GRAD_DTYPES, ids=IDS)
def test_value_determinism_identity(model, dtype):
    x, y = make_inputs(R.GRAD_CASES[1])
    x, y = x.to(DEV), y.to(DEV)
    wts = R.pair_weights(x.shape[0])
    val, g1 = _grad(model, x, y, dtype, wts)
    _, g2 = _grad(model, x, y, dtype, wts)
    model.set_compute_dtype(dtype)
    try:
        want = model(x, y)
        plain = model.forward_with_grad(x, y)                              # nobody asks for a gradient: the plain value
    finally:
        model.set_compute_dtype(torch.float32)
    assert val.shape == want.shape == (x.shape[0], 1, 1, 1) and torch.equal(val, want)
    assert not plain.requires_grad and torch.equal(plain, want)
    assert torch.equal(g1, g2) and bool((g1 != 0).any())
    v0, g0 = _grad(model, x, x.clone(), dtype, wts)
    assert bool((v0 == 0).all()) and bool((g0 == 0).all())


def test_autocast_runs_bf16_kernels(model):
    x, y = make_inputs(R.GRAD_CASES[0])
    x, y = x.to(DEV), y.to(DEV)
    val_w, g_w = _grad(model, x, y, torch.bfloat16)
    yy = y.clone().requires_grad_(True)
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        val = model.forward_with_grad(x, yy)
    assert model.last_dtype == torch.bfloat16 and val.dtype == torch.float32
    val.sum().backward()                                                   # outside the region: the pass keeps its arithmetic
    assert torch.equal(val.detach(), val_w) and torch.equal(yy.grad, g_w)
    with torch.autocast(device_type="cuda", dtype=torch.float16):
        with pytest.raises(NotImplementedError, match="float32 or bfloat16"):
            model.forward_with_grad(x, yy)


# ---- 5. chained with the decoder's backward --------------------------------------------------------------------------------------
def test_chain_with_decode_with_grad(model):
    from util import build_model

    vt, _, _ = build_model("vidtok_kl_causal_488_4chn", seed=7, device=DEV, dtype=torch.float32)
    x = (torch.rand(1, 3, 5, 32, 32, generator=torch.Generator().manual_seed(4)) * 2 - 1).to(DEV)
    torch.manual_seed(1)
    z = vt.encode(x)
    p = vt.decoder.conv_out.conv.weight

    def run(two_step):
        zz = z.detach().clone().requires_grad_(True)
        p.grad = None
        xh = vt.decode_with_grad(zz)
        assert xh.shape == x.shape
        if two_step:
            leaf = xh.detach().requires_grad_(True)
            model.forward_with_grad(frames(x), frames(leaf)).mean().backward()
            xh.backward(leaf.grad)
        else:
            model.forward_with_grad(frames(x), frames(xh)).mean().backward()
        return zz.grad.clone(), p.grad.clone()

    dz, dp = run(False)
    dz2, dp2 = run(True)
    for g in (dz, dp):
        assert bool(torch.isfinite(g).all()) and bool((g != 0).any())
    assert torch.equal(dz, dz2) and torch.equal(dp, dp2)
