"""GPU tests of the backward building blocks (vt_conv_wgrad, vt_layernorm_act_backward) against torch autograd on the CPU,
and of the graph cache after an in-place parameter update."""
import pytest
import torch
import torch.nn.functional as F

from util import build_model, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _virtual_input(x, g, tmode):
    """the tensor the forward convolution slides over: x NDHWC -> NCDHW, nearest x2 up-sampled, padded"""
    from vidtok_amd import lib as L

    v = x.permute(0, 4, 1, 2, 3)
    if g.ups_t:
        v = v.repeat_interleave(2, dim=2)
    if g.ups_s:
        v = v.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)
    if g.pt:
        front = v[:, :, :1].expand(-1, -1, g.pt, -1, -1) if tmode == L.VT_TPAD_REPLICATE else torch.zeros_like(v[:, :, :1]).expand(-1, -1, g.pt, -1, -1)
        v = torch.cat([front, v], dim=2)
    return F.pad(v, (g.pw, g.pw_hi, g.ph, g.ph_hi, 0, g.pt_hi))


def _ref_wgrad(x, dy, g, cin, cout, tmode, ref_dtype=torch.float64):
    """(dW, db) by torch autograd on the CPU (fp64 unless asked otherwise), from the same (rounded) operands the kernel reads"""
    xv = _virtual_input(x.cpu().to(ref_dtype), g, tmode)[:, :cin]
    w = torch.zeros((cout, cin, g.kt, g.kh, g.kw), dtype=ref_dtype, requires_grad=True)
    b = torch.zeros((cout,), dtype=ref_dtype, requires_grad=True)
    y = F.conv3d(xv, w, b, stride=(g.st, g.sh, g.sw))
    dyc = dy.cpu().to(ref_dtype)[..., :cout].permute(0, 4, 1, 2, 3)
    assert y.shape == dyc.shape, (y.shape, dyc.shape)
    (y * dyc).sum().backward()
    return w.grad, b.grad


def _geoms():
    from vidtok_amd.ops import ConvGeom

    return {
        "3x3x3": ConvGeom(kt=3, kh=3, kw=3, pt=2, ph=1, pw=1, ph_hi=1, pw_hi=1),
        "3x1x1": ConvGeom(kt=3, pt=2),
        "1x3x3": ConvGeom(kh=3, kw=3, ph=1, pw=1, ph_hi=1, pw_hi=1),
        "1x1x1": ConvGeom(),
        "up_s 1x3x3": ConvGeom(kh=3, kw=3, ph=1, pw=1, ph_hi=1, pw_hi=1, ups_s=1),
        "up_t 3x3x3": ConvGeom(kt=3, kh=3, kw=3, pt=2, ph=1, pw=1, ph_hi=1, pw_hi=1, ups_t=1),
    }


# (geometry, cin, stored cin, cout): conv_in (z 4 stored 8), conv_out (Cout 3), the C = 128 / 512 layers, odd channel counts
CASES = [("3x3x3", 4, 8, 128), ("3x3x3", 128, 128, 3), ("3x3x3", 128, 128, 128), ("3x1x1", 128, 128, 128), ("3x1x1", 512, 512, 512),
         ("1x3x3", 3, 8, 4), ("1x3x3", 8, 8, 512), ("1x1x1", 512, 512, 512), ("1x1x1", 128, 128, 8), ("up_s 1x3x3", 128, 128, 128),
         ("up_t 3x3x3", 8, 8, 8)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("gname,cin,ldx,cout", CASES)
def test_conv_wgrad_matches_autograd(gname, cin, ldx, cout, dtype):
    """dW / db of every decoder convolution shape, M (here 2 x 3 x 5 x 7 = 210 output pixels, or 4x that up-sampled) not a
    multiple of the tile; pad channels of x carry garbage that must not reach dW"""
    from vidtok_amd import lib as L
    from vidtok_amd import ops

    g = _geoms()[gname]
    gen = torch.Generator().manual_seed(cin * 7 + cout)
    B, T, H, W = 2, 3, 5, 7
    x = torch.randn((B, T, H, W, ldx), generator=gen)
    To, Ho, Wo = g.out_dims(T, H, W)
    ldy = ops.pad_channels(cout)
    dy = torch.randn((B, To, Ho, Wo, ldy), generator=gen)
    x, dy = x.to(dtype), dy.to(dtype)
    for tmode in ([L.VT_TPAD_ZERO, L.VT_TPAD_REPLICATE] if g.pt else [L.VT_TPAD_ZERO]):
        dw, db = ops.conv_wgrad(x.to(DEV), dy.to(DEV), g, cin=cin, cout=cout, tmode=tmode)
        rw, rb = _ref_wgrad(x, dy, g, cin, cout, tmode)
        assert dw.shape == rw.shape and dw.dtype == torch.float32
        assert rel_err(dw, rw) <= 1e-5, (gname, tmode, rel_err(dw, rw))
        assert rel_err(db, rb) <= 1e-5, (gname, tmode, rel_err(db, rb))


def test_conv_wgrad_bit_reproducible_and_without_bias():
    """a split reduction over many pixel ranges (the C = 128 3x3x3 layer on 2 x 17 x 32 x 32) gives the same bits every time"""
    from vidtok_amd import ops

    g = _geoms()["3x3x3"]
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((2, 17, 32, 32, 128), generator=gen).to(DEV, torch.bfloat16)
    dy = torch.randn((2, 17, 32, 32, 128), generator=gen).to(DEV, torch.bfloat16)
    a = ops.conv_wgrad(x, dy, g, cin=128, cout=128)
    b = ops.conv_wgrad(x, dy, g, cin=128, cout=128)
    c, none = ops.conv_wgrad(x, dy, g, cin=128, cout=128, bias=False)
    assert none is None
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], c)
    rw, rb = _ref_wgrad(x, dy, g, 128, 128, 0)
    assert rel_err(a[0], rw) <= 1e-5 and rel_err(a[1], rb) <= 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv_wgrad_many_ranges_with_partial_last_stage(dtype):
    """2 x 17 x 31 x 31 output pixels at C = 128 (3x3x3, replicate front pad): the reduction is split over many pixel ranges
    and the last range ends inside a 32-pixel stage"""
    from vidtok_amd import lib as L
    from vidtok_amd import ops

    g = _geoms()["3x3x3"]
    gen = torch.Generator().manual_seed(17)
    x = torch.randn((2, 17, 31, 31, 128), generator=gen).to(dtype)
    dy = torch.randn((2, 17, 31, 31, 128), generator=gen).to(dtype)
    assert (2 * 17 * 31 * 31) % 32 != 0
    d = ops.wgrad_desc(x, dy, g, cin=128, cout=128, tmode=L.VT_TPAD_REPLICATE)
    assert L.load().vt_conv_wgrad_work_bytes(d) >= 4 * 128 * 27 * 128 * 4       # at least four ranges of partial tiles
    dw, db = ops.conv_wgrad(x.to(DEV), dy.to(DEV), g, cin=128, cout=128, tmode=L.VT_TPAD_REPLICATE)
    rw, rb = _ref_wgrad(x, dy, g, 128, 128, L.VT_TPAD_REPLICATE, ref_dtype=torch.float32)
    assert rel_err(dw, rw) <= 1e-5 and rel_err(db, rb) <= 1e-5, (rel_err(dw, rw), rel_err(db, rb))


def _ref_ln(y, dn, gamma, beta, c, silu, eps):
    yv = y.double().cpu()[..., :c].clone().requires_grad_(True)
    gm = gamma.double().cpu().clone().requires_grad_(True)
    bt = beta.double().cpu().clone().requires_grad_(True)
    n = F.layer_norm(yv, (c,), gm, bt, eps)
    if silu:
        n = F.silu(n)
    (n * dn.double().cpu()[..., :c]).sum().backward()
    return yv.grad, gm.grad, bt.grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("c,ld,silu", [(4, 8, True), (128, 128, True), (128, 128, False), (256, 256, True), (512, 512, True),
                                       (3, 8, False)])
def test_layernorm_act_backward_matches_autograd(c, ld, silu, dtype):
    from vidtok_amd import ops

    gen = torch.Generator().manual_seed(c + ld + silu)
    shape = (2, 3, 5, 7, ld)
    y = (0.5 + 2.0 * torch.randn(shape, generator=gen)).to(dtype)
    dn = torch.randn(shape, generator=gen).to(dtype)
    gamma = 1.0 + 0.1 * torch.randn((c,), generator=gen)
    beta = 0.1 * torch.randn((c,), generator=gen)
    rdx, rg, rb = _ref_ln(y, dn, gamma, beta, c, silu, 1e-6)
    for dx_dtype in ({torch.float32, dtype}):
        dx, dg, db = ops.layernorm_act_backward(y.to(DEV), dn.to(DEV), gamma.to(DEV), beta.to(DEV), silu=silu, c=c, dx_dtype=dx_dtype)
        assert dx.dtype == dx_dtype and dx.shape == shape
        tol = 1e-5 if dx_dtype == torch.float32 else 1e-2        # a bf16 dx is rounded once
        assert rel_err(dx[..., :c], rdx) <= tol, rel_err(dx[..., :c], rdx)
        if ld > c:
            assert torch.count_nonzero(dx[..., c:]) == 0
        assert rel_err(dg, rg) <= 1e-5 and rel_err(db, rb) <= 1e-5, (rel_err(dg, rg), rel_err(db, rb))
    again = ops.layernorm_act_backward(y.to(DEV), dn.to(DEV), gamma.to(DEV), beta.to(DEV), silu=silu, c=c, dx_dtype=dx_dtype)
    assert all(torch.equal(a, b) for a, b in zip((dx, dg, db), again))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_graphed_decode_sees_in_place_weight_update(dtype):
    """train-then-evaluate: after an optimizer-style in-place update of decoder parameters, a graph-replayed decode must use
    the new weights -- bit-equal to an eager decode -- without an explicit invalidate_graphs()"""
    model, _cfg, _sd = build_model("vidtok_kl_causal_488_4chn", seed=21, device=DEV, dtype=dtype)
    z = torch.randn((1, 4, 3, 8, 8), generator=torch.Generator().manual_seed(3)).to(DEV)
    model.enable_graphs()
    before = [model.decode(z) for _ in range(3)]           # eager, capture, replay
    assert torch.equal(before[0], before[2])
    opt = torch.optim.SGD(model.decoder.parameters(), lr=0.05)
    for p in model.decoder.parameters():
        p.grad = torch.ones_like(p)
    opt.step()                                             # in place: parameter versions move, addresses do not
    after = [model.decode(z) for _ in range(3)]
    model.use_graphs = False
    eager = model.decode(z)
    assert not torch.equal(after[0], before[0])
    assert all(torch.equal(a, eager) for a in after)
    model.use_graphs = True
    assert torch.equal(model.decode(z), eager)
    assert isinstance(next(iter(model._gdec.entries.values())), tuple)     # replaying again once the weights hold still
