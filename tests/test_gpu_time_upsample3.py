"""`-m gpu`: vt_time_upsample3, the causal v1.0 time up-sampler as three frame products for two output frames (U = [W0 | W2] x shared by
the frames of a pair, V = W1 x shared by neighbouring pairs; one paired launch behind a plain convolution for V).

The operator tests compare with an fp32 host statement of the WHOLE up-sampler -- every frame twice, the causal 27-tap convolution, the
alpha-mix, the LayerNorm of the unrounded rows -- on the same 16-bit operands; V is never rounded there.  Gates: the operator gates of
tests/test_gpu_ops.py, TOL[dtype] for y and 2 TOL[dtype] for n.  The one rounding the paired form adds (V is stored in the 16-bit type)
was emulated on the CPU with these inputs (randn activations, weights randn / sqrt(27 C), alpha = sigmoid(0.2)): y and n after storage
rounding lie 3.2e-3 ... 4.6e-3 (bf16) and 4.1e-4 ... 8.6e-4 (fp16) from the statement, at most 0.6 of the gate."""
import math

import pytest
import torch
import torch.nn.functional as F

import torch_ops_ref as R  # noqa: F401  (the host statements the operator gates belong to)
from test_gpu_ops import TOL, _act
from util import build_model, rel_err, tup3_operands, tup3_run
from vidtok_amd import modules, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
H16 = [torch.bfloat16, torch.float16]
H16_IDS = ["bf16", "f16"]


def _statement(x, w, bias, mf, ln, dtype):
    """fp32: alpha up(x) + (1 - alpha) causal_conv3d(up(x)), up = every frame twice, on the operands as stored (x in `dtype`, every weight tap
    rounded to `dtype` once); ln = (gamma, beta, eps, silu) -> also the LayerNorm of the unrounded result.  NDHWC in, NDHWC fp32 out."""
    xf = x.detach().float().cpu().permute(0, 4, 1, 2, 3)
    up = xf.repeat_interleave(2, dim=2)
    c = F.conv3d(F.pad(up, (1, 1, 1, 1, 2, 0)), w.to(dtype).float(), bias.float().cpu())
    a = torch.sigmoid(mf.float().cpu())
    y = (a * up + (1 - a) * c).permute(0, 2, 3, 4, 1)
    if ln is None:
        return y, None
    gam, bet, eps, silu = ln
    n = F.layer_norm(y, (y.shape[-1],), gam.float().cpu(), bet.float().cpu(), eps)
    return y, (n * torch.sigmoid(n) if silu else n)


@pytest.mark.parametrize("silu", [False, True], ids=["ln", "ln_silu"])
@pytest.mark.parametrize("dtype", H16, ids=H16_IDS)
def test_paired_launch_with_layernorm(dtype, silu, vt_opts):
    """B = 2, T = 3, one tile per frame: the j = 0 tile of clip 1 must see V[-1] = 0 and not clip 0's last frame, the j = 0 tiles skip
    their zero time tap, both frames of a pair come interleaved out of one accumulator row, each with its own LayerNorm"""
    vt_opts(conv_tile=256)
    C = 256
    x, w, bias, wu, wv, mf, gam, bet = tup3_operands(2, 3, 16, 16, C, dtype)
    ln = (gam, bet, 1e-6, silu)
    y, n, v = tup3_run(x, bias, wu, wv, mf, ln, C)
    yr, nr = _statement(x, w, bias, mf, ln, dtype)
    assert torch.isfinite(y.float()).all() and torch.isfinite(n.float()).all()
    ey, en = rel_err(y, yr), rel_err(n, nr)
    print(f"time_upsample3 {dtype} silu={silu}: y {ey:.3e} n {en:.3e}")
    assert ey < TOL[dtype] and en < 2 * TOL[dtype], (ey, en)
    # the clip boundary on its own: frame 0 of clip 1 (V[-1] = 0) against the statement, and apart from what clip 0's last V would give
    e0 = rel_err(y[1, 0], yr[1, 0])
    assert e0 < TOL[dtype], e0
    a = torch.sigmoid(mf.float().cpu())
    leaked = yr[1, 0] + (1 - a) * v[0, -1].float().cpu()           # what a launch that took clip 0's last V for V[-1] would write
    # (V has standard deviation sqrt(9 C / 27 C) = 0.58, so the leaked term peaks near 0.45 * 4 * 0.58 = 1 against outputs peaking near 4)
    assert rel_err(y[1, 0], leaked) > 0.05, rel_err(y[1, 0], leaked)


@pytest.mark.parametrize("silu", [True, False], ids=["ln_silu", "ln"])
@pytest.mark.parametrize("dtype", H16, ids=H16_IDS)
def test_paired_launch_with_zero_v_is_the_plain_launch(dtype, silu, vt_opts):
    """V = 0: both frames of a pair are alpha x[j] + (1 - alpha) (U[j] + bias + 0), which is what a plain ops.conv of the same [W0 | W2]
    rows with the alpha-mix against x and the same LayerNorm writes -- t + 0 is exact and the paired epilogue finishes a row with the
    row phase of the 256-wide tile's plain one, so y and n are the plain launch's bit for bit (B = 2, T = 3, one tile = one frame)"""
    from vidtok_amd import lib as L

    vt_opts(conv_tile=256)
    C = 256
    x, _w, bias, wu, _wv, mf, gam, bet = tup3_operands(2, 3, 16, 16, C, dtype)
    ln = (gam, bet, 1e-6, silu)
    y = torch.full((2, 6, 16, 16, C), float("nan"), dtype=dtype, device=DEV)
    n = torch.full_like(y, float("nan"))
    r = ops.time_upsample3(x, (wu, bias), torch.zeros_like(x), mf, y, cout=C, ln=ln, ln_out=n)
    assert isinstance(r, tuple), "the paired launch serves this shape and takes the LayerNorm"
    ops.CONV_RECORD = []
    try:
        y_plain, n_plain = ops.conv(x, wu, bias, ops.TUP3_GEOM, cout=C, res=x, res_mode=L.VT_RES_MIX, mix_factor=mf, ln=ln)
        plan = ops.conv_plan(ops.CONV_RECORD[0][0])
    finally:
        ops.CONV_RECORD = None
    torch.cuda.synchronize()
    assert plan["kernel"] == "igemm" and plan["tile"] == (256, 256) and plan["ln_fused"], plan
    assert torch.isfinite(n_plain.float()).all()
    for q in (0, 1):
        assert torch.equal(y[:, q::2], y_plain), f"y, frames 2j + {q}"
        assert torch.equal(n[:, q::2], n_plain), f"n, frames 2j + {q}"


@pytest.mark.parametrize("dtype", H16, ids=H16_IDS)
def test_paired_launch_two_channel_tiles(dtype, vt_opts):
    """512 -> 512 on 16 x 32 frames without LayerNorm: two channel tiles (the channel offset into V and x) and two pixel tiles per frame"""
    vt_opts(conv_tile=256)
    C = 512
    x, w, bias, wu, wv, mf, _g, _b = tup3_operands(1, 2, 16, 32, C, dtype)
    y, n, _ = tup3_run(x, bias, wu, wv, mf, None, C)
    yr, _ = _statement(x, w, bias, mf, None, dtype)
    assert torch.isfinite(y.float()).all()
    e = rel_err(y, yr)
    print(f"time_upsample3 512 {dtype}: y {e:.3e}")
    assert e < TOL[dtype], e


@pytest.mark.parametrize("dtype", H16, ids=H16_IDS)
def test_paired_launch_single_frame(dtype, vt_opts):
    """T = 1: both output frames come from j = 0 (no V[j-1] anywhere)"""
    vt_opts(conv_tile=256)
    C = 256
    x, w, bias, wu, wv, mf, _g, _b = tup3_operands(1, 1, 16, 16, C, dtype)
    y, _, _ = tup3_run(x, bias, wu, wv, mf, None, C)
    yr, _ = _statement(x, w, bias, mf, None, dtype)
    assert torch.isfinite(y.float()).all()
    e = rel_err(y, yr)
    assert e < TOL[dtype], e


def _upsampler(C, seed=3):
    torch.manual_seed(seed)
    m = modules.TimeUpsampleResCausal2x(C, C, mix_factor=0.2)
    with torch.no_grad():
        m.conv.conv.weight.copy_(torch.randn_like(m.conv.conv.weight) / math.sqrt(27 * C))
        m.conv.conv.bias.copy_(torch.randn_like(m.conv.conv.bias) * 0.1)
    norm = modules.LayerNorm(C)
    with torch.no_grad():
        norm.norm.weight.copy_(torch.randn(C) * 0.5 + 1.0)
        norm.norm.bias.copy_(torch.randn(C) * 0.2)
    return m.to(DEV), norm.to(DEV)


def _module_run(m, x, dt, next_norm):
    """(result, number of paired launches it took)"""
    ops.CONV_RECORD = []
    try:
        r = m.run(x, dt, next_norm)
        torch.cuda.synchronize()
        return r, sum(isinstance(d, ops.TimeUp3Desc) for d, _k, _l in ops.CONV_RECORD)
    finally:
        ops.CONV_RECORD = None


@pytest.mark.parametrize("shape,dtype", [((2, 3, 8, 8), torch.bfloat16), ((1, 2, 16, 16), torch.float32)], ids=["8x8_frames", "fp32"])
def test_refused_shapes_fall_back_bit_for_bit(shape, dtype, vt_opts):
    """64 pixels per frame (a tile would span frames) and fp32 storage: supported == 0, the module runs the two parity launches -- the bits
    of option conv_tup3 = 0"""
    vt_opts(conv_tile=256)
    C = 256
    m, norm = _upsampler(C)
    x, _w, _bias, _wu, _wv, mf, _g, _b = tup3_operands(*shape, C, dtype)
    y = torch.empty((shape[0], 2 * shape[1]) + shape[2:] + (C,), dtype=dtype, device=DEV)
    refused = lambda: pytest.fail("nothing is packed or computed for a refused launch")      # noqa: E731
    assert ops.time_upsample3(x, refused, refused, mf, y, cout=C) is None             # (fp32: the library itself answers no)
    on, k_on = _module_run(m, x, dtype, (norm, True))
    vt_opts(conv_tup3=0)
    off, k_off = _module_run(m, x, dtype, (norm, True))
    assert k_on == 0 and k_off == 0
    assert type(on) is type(off)
    for a, b in ((on.y, off.y), (on.n, off.n)) if isinstance(on, modules.Normed) else ((on, off),):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", H16, ids=H16_IDS)
def test_module_paired_against_parity_launches(dtype, vt_opts):
    """TimeUpsampleResCausal2x(256, 256) with option conv_tup3 on (V + one paired launch) and off (the two parity launches): the same
    operator under one more rounding, so closer than the operator gate; with conv_tup_ln = 0 the paired launch emits no LayerNorm"""
    vt_opts(conv_tile=256)
    C = 256
    m, norm = _upsampler(C)
    x = _act(2, 3, 16, 16, C, dtype, 5)
    on, k_on = _module_run(m, x, dtype, (norm, True))
    assert k_on == 1 and isinstance(on, modules.Normed) and on.norm is norm and on.silu is True
    plain, k_plain = _module_run(m, x, dtype, None)
    assert k_plain == 1 and isinstance(plain, torch.Tensor) and torch.equal(plain, on.y)
    vt_opts(conv_tup3=0)
    off, k_off = _module_run(m, x, dtype, (norm, True))
    assert k_off == 0 and isinstance(off, modules.Normed)
    ey, en = rel_err(on.y, off.y), rel_err(on.n, off.n)
    print(f"module on/off {dtype}: y {ey:.3e} n {en:.3e}")
    assert ey < TOL[dtype] and en < TOL[dtype], (ey, en)
    vt_opts(conv_tup3=1, conv_tup_ln=0)
    noln, k_noln = _module_run(m, x, dtype, (norm, True))
    assert k_noln == 1 and isinstance(noln, torch.Tensor) and torch.equal(noln, on.y)


def test_engine_and_model_handle_take_the_paired_path(vt_opts):
    """bf16 vidtok_kl_causal_488_4chn on one 5 x 64 x 64 clip with the 8-wave tile forced: both time up-samplers of the decoder run as V +
    paired launch in the Python engine, the vt_model handle (csrc/model.cpp) makes the same decision and gives the same bits; the encoder
    does not know the option -- z is the conv_tup3 = 0 run's z bit for bit (the decoder's distance between the two forms is printed)"""
    from test_gpu_e2e import _handle_vs_engine

    dtype = torch.bfloat16
    shape = (1, 3, 5, 64, 64)
    vt_opts(conv_tile=256)
    model, cfg, sd = build_model("vidtok_kl_causal_488_4chn", device=DEV, dtype=dtype)
    torch.manual_seed(5)
    x = (torch.rand(shape, device=DEV) * 2 - 1).contiguous()
    h_on = model._run_encoder(x)
    z = ops.kl_sample(h_on.contiguous(), None)[0]
    ops.CONV_RECORD = []
    try:
        dec_on = model._run_decoder(z)
        torch.cuda.synchronize()
        paired = sum(isinstance(d, ops.TimeUp3Desc) for d, _k, _l in ops.CONV_RECORD)
    finally:
        ops.CONV_RECORD = None
    assert paired == 2, paired
    _handle_vs_engine(model, cfg, sd, shape, dtype)               # encoder, regularizer and decoder of the handle: the engine's bits
    vt_opts(conv_tup3=0)
    h_off = model._run_encoder(x)
    dec_off = model._run_decoder(z)
    torch.cuda.synchronize()
    assert torch.equal(h_on, h_off)
    e = rel_err(dec_on, dec_off)
    print(f"decoder, conv_tup3 on vs off: {e:.3e}")
