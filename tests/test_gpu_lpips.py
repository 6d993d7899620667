"""LPIPS on the MI355X: vt_conv_act per tile class and arithmetic, the fused tap head + max-pool, the whole pass against the golden
values of the unmodified reference and against the pure-torch restatement (tests/lpips_ref.py), and its properties (exact zero on
identical images, symmetry, determinism, graph replay, the eval-loop helper, autocast)."""
import math
import os

import pytest
import torch
import torch.nn.functional as F
from safetensors.torch import load_file

import lpips_ref
from lpips_cases import CASES, lpips_state_dict, make_inputs
from util import GOLDEN_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# 16-bit gates of the whole pass, max relative distance per pair to the golden / fp32 restatement: 2x the largest distance measured over
# the cases of this file on an MI355X (bf16 5.87e-4 on p2_32, fp16 6.25e-5 on p2_32; fp32 measured 2.3e-7)
GATE = {torch.float32: 1e-4, torch.bfloat16: 1.2e-3, torch.float16: 1.3e-4}
# vt_conv_act against the fp64 convolution of the same (rounded) operands, max |d| / max |ref|: the rounding of the result to the
# storage type dominates (bf16 2^-9, fp16 2^-12 of the value)
CONV_GATE = {torch.float32: 1e-5, torch.bfloat16: 8e-3, torch.float16: 1e-3}


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.fixture(scope="module")
def model(built_lib):
    from vidtok_amd.lpips import LPIPS

    m = LPIPS(pretrained=False)
    m.load_state_dict(lpips_state_dict({k: v.shape for k, v in m.state_dict().items()}), strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def sd_dev(model):
    return {k: v.to(DEV) for k, v in model.state_dict().items()}


# ---- vt_conv_act ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("cin, cout, hw", [(3, 64, (20, 24)), (64, 64, (16, 16)), (64, 128, (16, 20)), (128, 256, (16, 16)),
                                           (256, 512, (12, 10))], ids=["in3_64", "64_64", "64_128", "128_256", "256_512"])
def test_conv_act_matches_relu_conv(built_lib, dtype, cin, cout, hw):
    from vidtok_amd import ops
    from vidtok_amd.lpips import _GEOM3

    g = torch.Generator().manual_seed(cin * 7 + cout)
    N, (H, W) = 3, hw
    x = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
    b = 0.1 * torch.randn(cout, generator=g)
    cs = 8 if cin == 3 else cin
    xs = torch.zeros(N, 1, H, W, cs, dtype=dtype)
    xs[..., :cin] = x.permute(0, 2, 3, 1).unsqueeze(1).to(dtype)
    wp = ops.pack_conv_weight(w.to(DEV), dtype, cin_stored=cs)
    y = ops.conv_act(xs.to(DEV), wp, b.to(DEV), _GEOM3, cout=cout)
    ref = F.relu(F.conv2d(xs[:, 0, ..., :cin].permute(0, 3, 1, 2).double(), w.to(dtype).double(), b.double(), padding=1))
    got = y[:, 0].permute(0, 3, 1, 2).cpu()
    assert got.dtype == dtype and bool((got >= 0).all())
    print(f"[conv_act] {cin}->{cout} {dtype}: rel {_rel(got, ref):.3e}")
    assert _rel(got, ref) <= CONV_GATE[dtype], _rel(got, ref)


# ---- vt_lpips_tap ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("C, H, W", [(64, 13, 9), (128, 8, 8), (256, 7, 6), (512, 3, 2), (512, 5, 3)])
def test_tap_head_and_pool(built_lib, dtype, C, H, W):
    from vidtok_amd import ops

    g = torch.Generator().manual_seed(C + H * 31 + W)
    N = 3
    feat = F.relu(torch.randn(2 * N, H, W, C, generator=g)).to(dtype)
    feat[1, 0, 0] = 0.0                                       # an all-zero pixel: the norm's eps path
    lw = torch.rand(C, generator=g)
    work = torch.zeros(5 * N * 64, dtype=torch.float32, device=DEV)
    fd = feat.to(DEV)
    pooled = ops.lpips_tap(fd, lw.to(DEV), work, tap=2, pool=True)
    torch.cuda.synchronize()
    want_pool = F.max_pool2d(fd.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert pooled.shape == want_pool.shape and torch.equal(pooled, want_pool)       # bit-equal, odd sizes floored
    f = feat.permute(0, 3, 1, 2).double()
    d = (lpips_ref.normalize_tensor(f[:N]) - lpips_ref.normalize_tensor(f[N:])) ** 2
    want = (d * lw.double()[None, :, None, None]).sum(1).sum([1, 2])
    got = work.view(5, N, 64)[2].sum(-1).cpu()
    assert _rel(got, want) <= 1e-5


# ---- the whole pass -------------------------------------------------------------------------------------------------------------
def _ours(model, case, dtype):
    x, y = make_inputs(case)
    model.set_compute_dtype(dtype)
    try:
        if case["form"] == "eval":
            return model.frames(x.to(DEV), y.to(DEV)).reshape(-1).cpu()
        return model(x.to(DEV), y.to(DEV)).reshape(-1).cpu()
    finally:
        model.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_lpips_vs_golden_and_restatement(model, sd_dev, case, dtype):
    g = load_file(os.path.join(GOLDEN_DIR, "lpips.safetensors"))[case["name"] + "/lpips"]
    got = _ours(model, case, dtype)
    x, y = make_inputs(case)
    with torch.no_grad():
        r = (lpips_ref.eval_frames(sd_dev, x.to(DEV), y.to(DEV)) if case["form"] == "eval" else lpips_ref.lpips(sd_dev, x.to(DEV), y.to(DEV)))
    r = r.reshape(-1).cpu()
    e_g, e_r = ((got - g).abs() / g.abs()).max().item(), ((got - r).abs() / r.abs()).max().item()
    print(f"[lpips] {case['name']} {dtype}: max rel vs golden {e_g:.3e}, vs restatement {e_r:.3e}")
    assert e_g <= GATE[dtype] and e_r <= GATE[dtype], (e_g, e_r)


def test_lpips_256_four_pairs(model, sd_dev):
    g = torch.Generator().manual_seed(21)
    x = torch.rand(4, 3, 256, 256, generator=g) * 2 - 1
    y = (x + 0.2 * torch.randn(4, 3, 256, 256, generator=g)).clamp(-1, 1)
    x, y = x.to(DEV), y.to(DEV)
    got = model(x, y).reshape(-1)
    with torch.no_grad():
        want = lpips_ref.lpips(sd_dev, x, y)
    e = ((got - want).abs() / want.abs()).max().item()
    print(f"[lpips] 256x256 x 4 fp32: max rel vs restatement {e:.3e}")
    assert e <= GATE[torch.float32]


# ---- properties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_identity_symmetry_determinism(model, dtype):
    x, y = make_inputs(CASES[1])
    x, y = x.to(DEV), y.to(DEV)
    model.set_compute_dtype(dtype)
    try:
        assert bool((model(x, x) == 0).all())
        a, b, a2 = model(x, y), model(y, x), model(x, y)
    finally:
        model.set_compute_dtype(torch.float32)
    assert torch.equal(a, b) and torch.equal(a, a2) and bool((a > 0).all())


def test_graph_replay_bit_equal(model):
    x, y = make_inputs(CASES[2])
    x, y = x.to(DEV), y.to(DEV)
    eager = model.frames(x, y)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.frames(x, y)                                     # warm: packed weights exist before the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model.frames(x, y)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_evaluate_clip_lpips(model, sd_dev):
    from util import build_model

    from vidtok_amd import metrics

    vt, _, _ = build_model("vidtok_kl_causal_488_4chn", seed=7, device=DEV, dtype=torch.float32)
    x = (torch.rand(1, 3, 9, 64, 64, generator=torch.Generator().manual_seed(4)) * 2 - 1).to(DEV)
    torch.manual_seed(1)                                       # the KL posterior sample: same noise in both calls
    xrec0, p0, s0 = metrics.evaluate_clip(vt, x)
    torch.manual_seed(1)
    xrec, p, s, lp = metrics.evaluate_clip_lpips(vt, x, model)
    # the reconstruction is bit-equal; psnr / ssim come from the same vt_eval_psnr_ssim call on it, whose per-frame accumulation
    # (atomic adds of the workgroup sums) is not bit-reproducible from one call to the next, so they agree to summation order only
    assert torch.equal(xrec, xrec0)
    assert ((p - p0).abs().max() / p0.abs().max()).item() <= 1e-6 and ((s - s0).abs().max() / s0.abs().max()).item() <= 1e-6
    with torch.no_grad():
        want = lpips_ref.eval_frames(sd_dev, x, xrec)
    assert lp.shape == (1, 9)
    assert ((lp - want).abs() / want.abs()).max().item() <= 1e-4


def test_compute_lpips_unit_images(model, sd_dev):
    from vidtok_amd import metrics

    x, y = make_inputs(CASES[0])
    xi, yi = ((x + 1) / 2).to(DEV), ((y + 1) / 2).to(DEV)
    got = metrics.compute_lpips(xi, yi, model)
    with torch.no_grad():
        want = lpips_ref.lpips(sd_dev, xi * 2 - 1, yi * 2 - 1).mean()
    assert abs(got.item() - want.item()) <= 1e-4 * abs(want.item())


def test_autocast_runs_fp16_kernels(model):
    x, y = make_inputs(CASES[0])
    x, y = x.to(DEV), y.to(DEV)
    model.set_compute_dtype(torch.float16)
    try:
        want = model(x, y)
    finally:
        model.set_compute_dtype(torch.float32)
    with torch.autocast(device_type="cuda", dtype=torch.float16):
        got = model(x, y)
    assert model.last_dtype == torch.float16 and got.dtype == torch.float32
    assert torch.equal(got, want)
    model(x, y)
    assert model.last_dtype == torch.float32
