"""PatchGAN discriminator on the GPU: the new kernels one by one against fp64 computed from the same stored operands, ops.conv_wgrad at
the five layer geometries, arena runs of every new entry point, and the whole network (forward, both backward sides, the chain behind
decode_with_grad) against fp64 autograd of the torch.nn restatement (tests/patchgan_ref.py)."""
import dataclasses
import functools

import pytest
import torch
import torch.nn.functional as F

import arena as A
import patchgan_ref as R
from util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
IDS = ["f32", "bf16"]
SLOPE = 0.2
BN_SHAPES = [(20, 128, 128), (1512, 64, 64), (777, 20, 64), (2, 512, 512)]          # (M, C, ld)
BN_IDS = ["20x128", "1512x64", "777x20of64", "2x512"]


def _mods():
    from vidtok_amd import lib as L
    from vidtok_amd import ops

    return ops, L


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rows(M, C, ld, dtype, seed, scale=1.0, shift=0.0):
    """[M, ld] in `dtype`: the first C lanes seeded, finite garbage in the pad lanes"""
    x = torch.randn((M, ld), generator=_gen(seed)) * scale + shift
    x[:, C:] = 7.0
    return x.to(dtype)


# ---- 1. vt_batchnorm_stats ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("offset", [False, True], ids=["randn", "mean100"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=BN_IDS)
def test_batchnorm_stats(shape, offset, dtype):
    ops, _ = _mods()
    M, C, ld = shape
    x = _rows(M, C, ld, dtype, 1, 0.5 if offset else 1.0, 100.0 if offset else 0.0)
    xd = x.double()[:, :C]
    rm, rv = xd.mean(dim=0), xd.var(dim=0, unbiased=False)
    mean, var, rstd = ops.batchnorm_stats(x.to(DEV), c=C, eps=1e-5)
    again = ops.batchnorm_stats(x.to(DEV), c=C, eps=1e-5)
    em = float(((mean.double().cpu() - rm).abs() / rm.abs().clamp_min(1e-300)).max())
    ev = float(((var.double().cpu() - rv).abs() / rv.abs().clamp_min(1e-300)).max())
    er = float(((rstd.double().cpu() - (rv + 1e-5).rsqrt()).abs() * (rv + 1e-5).sqrt()).max())
    print(f"[bn stats] {shape} offset {offset} {dtype}: mean {em:.2e} var {ev:.2e} rstd {er:.2e}")
    assert em <= 1e-6 and ev <= 1e-5 and er <= 1e-5, (em, ev, er)
    assert all(torch.equal(a, b) for a, b in zip((mean, var, rstd), again))


# ---- 2. vt_batchnorm_act forward and backward ----------------------------------------------------------------------------------------
def _bn_case(shape, dtype, batch):
    """stored operands with a column whose pre-activation is exactly 0 (a constant column, beta 0) and a channel with gamma 0"""
    ops, _ = _mods()
    M, C, ld = shape
    x = _rows(M, C, ld, dtype, 2, 1.5, 0.3)
    x[:, 1] = torch.tensor(0.75).to(dtype)
    gamma, beta = 1.0 + 0.3 * torch.randn(C, generator=_gen(3)), 0.2 * torch.randn(C, generator=_gen(4))
    beta[1], gamma[2] = 0.0, 0.0
    if batch:
        mean, _var, rstd = (t.cpu() for t in ops.batchnorm_stats(x.to(DEV), c=C, eps=1e-5))
    else:
        mean, rstd = 0.3 + 0.2 * torch.randn(C, generator=_gen(5)), (0.5 + torch.rand(C, generator=_gen(6))).rsqrt()
        mean[1] = 0.75
    return x, mean, rstd, gamma, beta


def _bn_ref(x, dy, mean, rstd, gamma, beta, C, batch):
    xd, dyd = x.double()[:, :C], dy.double()[:, :C]
    m, r, g, b = mean.double(), rstd.double(), gamma.double(), beta.double()
    xh = (xd - m) * r
    pre = xh * g + b
    y = torch.where(pre > 0, pre, SLOPE * pre)
    gg = dyd * torch.where(pre > 0, 1.0, SLOPE)
    dbeta, dgamma = gg.sum(dim=0), (gg * xh).sum(dim=0)
    dx = g * r * (gg - dbeta / x.shape[0] - xh * dgamma / x.shape[0]) if batch else g * r * gg
    return y, dx, dgamma, dbeta, pre


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("batch", [True, False], ids=["batch", "running"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=BN_IDS)
def test_batchnorm_act_forward_backward(shape, batch, dtype):
    ops, _ = _mods()
    M, C, ld = shape
    x, mean, rstd, gamma, beta = _bn_case(shape, dtype, batch)
    dev = [t.to(DEV) for t in (x, mean, rstd, gamma, beta)]
    y = ops.batchnorm_act(*dev, SLOPE, c=C)
    dy32 = _rows(M, C, ld, F32, 7)
    ry, _, _, _, pre = _bn_ref(x, dy32, mean, rstd, gamma, beta, C, batch)
    assert bool((pre[:, 1] == 0).all()) and y.dtype == dtype
    ey = rel_err(y[:, :C], ry)
    assert ey <= (1e-5 if dtype == F32 else 2.0 ** -8), ey
    assert bool((y[:, C:] == 0).all()) and bool((y[:, 1] == 0).all())
    assert torch.equal(y, ops.batchnorm_act(*dev, SLOPE, c=C))
    for dyt in ([F32] if dtype == F32 else [BF16, F32]):
        dy = dy32.to(dyt)
        _, rdx, rg, rb, _ = _bn_ref(x, dy, mean, rstd, gamma, beta, C, batch)
        dx, dg, db = ops.batchnorm_act_backward(dev[0], dy.to(DEV), *dev[1:], SLOPE, batch=batch, c=C)
        torch.cuda.synchronize()
        es = (rel_err(dx[:, :C], rdx), rel_err(dg, rg), rel_err(db, rb))
        print(f"[bn bwd] {shape} batch {batch} {dtype} dy {dyt}: dx {es[0]:.2e} dgamma {es[1]:.2e} dbeta {es[2]:.2e}")
        assert dx.dtype == dtype and es[0] <= (1e-5 if dtype == F32 else 2.0 ** -8) and es[1] <= 1e-5 and es[2] <= 1e-5, es
        assert bool((dx[:, C:] == 0).all()) and bool((dx[:, 2] == 0).all())                     # pad lanes; gamma = 0
        # pre == 0 takes the slope: the gradient of the constant column's beta counts every row with `slope`
        assert abs(float(db[1]) - SLOPE * float(dy.double()[:, 1].sum())) <= 1e-5 * float(rb.abs().max())
        dx2, dg2, db2 = ops.batchnorm_act_backward(dev[0], dy.to(DEV), *dev[1:], SLOPE, batch=batch, c=C)
        assert torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2)
        dx3, none_g, none_b = ops.batchnorm_act_backward(dev[0], dy.to(DEV), *dev[1:], SLOPE, batch=batch, c=C, need_dgamma=False, need_dbeta=False)
        assert none_g is None and none_b is None and torch.equal(dx3, dx)


def test_first_layer_leaky_is_exact():
    """mean 0, rstd 1, gamma 1, beta 0: vt_batchnorm_act is a plain LeakyReLU, bit for bit"""
    ops, _ = _mods()
    for dtype in DTYPES:
        x = _rows(333, 64, 64, dtype, 8).to(DEV)
        z, o = torch.zeros(64, device=DEV), torch.ones(64, device=DEV)
        y = ops.batchnorm_act(x, z, o, o, z, SLOPE)
        assert torch.equal(y, torch.where(x > 0, x.float(), SLOPE * x.float()).to(dtype))


# ---- 3. vt_leaky_relu_backward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_leaky_relu_backward(dtype):
    ops, _ = _mods()
    big = torch.randn((6, 1, 13, 18, 64), generator=_gen(9)).to(dtype).to(DEV)
    big[0, 0, 0, 0, :8] = 0.0
    for y in (big, big[2:5]):                                                   # the whole tensor and a slice of a larger saved one
        for dyt in {dtype, F32}:
            dy = torch.randn(y.shape, generator=_gen(10)).to(dyt).to(DEV)
            dx = ops.leaky_relu_backward(dy, y, SLOPE)
            want = (dy.float() * torch.where(y > 0, 1.0, SLOPE)).to(dtype)
            assert dx.dtype == dtype and torch.equal(dx, want)


# ---- 4. vt_conv_dgrad under a row / column stride -------------------------------------------------------------------------------------------
def _strided_geoms():
    from backward_sites import edge_geoms
    from vidtok_amd.ops import ConvGeom

    return {"k4 s2 p1": ConvGeom(kh=4, kw=4, sh=2, sw=2, ph=1, pw=1, ph_hi=1, pw_hi=1), "downsample 3x3 s2": edge_geoms()["downsample 3x3 s2"][0],
            "1x3x3 s21": edge_geoms()["1x3x3 s21"][0]}


def _ref_strided_dx(dy, w, g, cin, cout, x_shape):
    B, T, H, W, _ = x_shape
    x = torch.zeros((B * T, cin, H, W), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.pad(x, (g.pw, g.pw_hi, g.ph, g.ph_hi)), w.double(), stride=(g.sh, g.sw))
    dyc = dy.cpu().double()[..., :cout].reshape(B * T, dy.shape[2], dy.shape[3], cout).permute(0, 3, 1, 2)
    assert y.shape == dyc.shape, (y.shape, dyc.shape)
    (y * dyc).sum().backward()
    return x.grad.permute(0, 2, 3, 1).reshape(B, T, H, W, cin)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("gname", ["k4 s2 p1", "downsample 3x3 s2", "1x3x3 s21"])
def test_conv_dgrad_strided(gname, dtype):
    """fp32 dx against fp64 autograd of F.conv2d (gate 1e-5, as the stride-1 grid), zero pad lanes, acc = a separate add bit for bit, a
    bf16 dx = the rounded fp32 dx (+ acc: one rounding of the fp32 sum); garbage in dy's pad lanes"""
    ops, _ = _mods()
    g = _strided_geoms()[gname]
    for dims in ((2, 1, 9, 12), (2, 1, 8, 7), (1, 3, 5, 6)):
        for cin, cout in ((12, 20), (3, 64), (128, 256)):
            B, T, H, W = dims
            _, Ho, Wo = g.out_dims(T, H, W)
            ldx, lddy = ops.pad_channels(cin), ops.pad_channels(cout)
            w = (torch.randn((cout, cin, g.kh, g.kw), generator=_gen(11)) * 0.2).to(dtype)          # the rounded weight both sides use
            dy = torch.randn((B, T, Ho, Wo, lddy), generator=_gen(12))
            dy[..., cout:] = 3.0
            dy = dy.to(dtype).to(DEV)
            ref = _ref_strided_dx(dy, w, g, cin, cout, (B, T, H, W, ldx))
            wt = ops.pack_conv_weight_dgrad(w.float().to(DEV), dtype, lddy, g)
            run = functools.partial(ops.conv_dgrad, dy, wt, g, cin=cin, cout=cout, in_hw=(H, W))
            dx = run(dx_dtype=F32)
            torch.cuda.synchronize()
            assert tuple(dx.shape) == (B, T, H, W, ldx) and dx.dtype == F32
            err = rel_err(dx[..., :cin], ref)
            print(f"[dgrad strided] {gname} {dims} {cin}->{cout} {dtype}: rel {err:.2e}")
            assert err <= 1e-5, (gname, dims, cin, cout, err)
            assert bool((dx[..., cin:] == 0).all()), "pad lanes of dx must be zero"
            assert torch.equal(dx, run(dx_dtype=F32))
            acc = torch.randn(dx.shape, generator=_gen(5)).to(DEV)
            dxa = run(dx_dtype=F32, acc=acc)
            assert torch.equal(dxa[..., :cin], (dx + acc)[..., :cin]) and bool((dxa[..., cin:] == 0).all())
            if dtype == BF16:
                dxh = run()
                assert dxh.dtype == BF16 and torch.equal(dxh, dx.to(BF16))
                acch = acc.to(BF16)
                dxha = run(acc=acch)
                assert torch.equal(dxha[..., :cin], (dx + acch.float()).to(BF16)[..., :cin])


def test_conv_dgrad_domain_of_the_wrapper():
    """ops.conv_dgrad on the GPU: a stride needs in_hw, what the library refuses raises with its message (host side of the domain:
    tests/test_patchgan_host.py::test_conv_dgrad_domain), stride 1 checks an in_hw it is given"""
    ops, L = _mods()
    g = _strided_geoms()["k4 s2 p1"]
    dy = torch.zeros((1, 1, 4, 4, 8), device=DEV)
    wt = ops.pack_conv_weight_dgrad(torch.zeros((8, 8, 4, 4), device=DEV), F32, 8, g)
    assert tuple(wt.shape) == (4, 8, 4 * 8)
    with pytest.raises(L.VtError, match="pass in_hw"):
        ops.conv_dgrad(dy, wt, g, cin=8, cout=8)
    with pytest.raises(L.VtError, match="are not the forward convolution's"):
        ops.conv_dgrad(dy, wt, g, cin=8, cout=8, in_hw=(11, 8))
    with pytest.raises(L.VtError, match="zero time pad"):
        ops.conv_dgrad(dy, wt, g, cin=8, cout=8, in_hw=(8, 8), tmode=L.VT_TPAD_REPLICATE)
    with pytest.raises(L.VtError, match="strides"):
        ops.conv_dgrad(dy, wt, dataclasses.replace(g, sh=3), cin=8, cout=8, in_hw=(8, 8))
    assert float(ops.conv_dgrad(dy, wt, g, cin=8, cout=8, in_hw=(8, 8)).abs().max()) == 0
    g1 = ops.ConvGeom(kh=4, kw=4, ph=1, pw=1, ph_hi=1, pw_hi=1)
    dy1, wt1 = torch.zeros((1, 1, 7, 7, 8), device=DEV), ops.pack_conv_weight_dgrad(torch.zeros((8, 8, 4, 4), device=DEV), F32, 8)
    assert tuple(wt1.shape) == (8, 16 * 8) and tuple(ops.conv_dgrad(dy1, wt1, g1, cin=8, cout=8, in_hw=(8, 8)).shape) == (1, 1, 8, 8, 8)
    with pytest.raises(AssertionError):
        ops.conv_dgrad(dy1, wt1, g1, cin=8, cout=8, in_hw=(9, 8))


# ---- 5. arena: every new entry point reads and writes only inside its operands --------------------------------------------------------------
def _direct(names, run, operands, scratch=None):
    _, L = _mods()
    with A.CallLog(*names) as calls:
        out = run()
    torch.cuda.synchronize()
    assert calls, names
    ar, new = A.relocate_calls(calls, L.SIGNATURES, operands(out), scratch)
    lib = L.load()
    for name, args in new:
        L.check(getattr(lib, name)(*args), name)
    torch.cuda.synchronize()
    ar.check()
    return ar


def _in(name, t):
    return dict(name=name, t=t)


def _out(name, t, **kw):
    return dict(name=name, t=t, kind="out", **kw)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_arena_batchnorm_and_leaky(dtype):
    ops, L = _mods()
    M, C, ld = 777, 20, 64
    x, mean, rstd, gamma, beta = (t.to(DEV) for t in _bn_case((M, C, ld), dtype, False))
    chan = [_in("mean", mean), _in("rstd", rstd), _in("gamma", gamma), _in("beta", beta)]
    nb = L.load().vt_batchnorm_stats_work_bytes(M, C)
    _direct(["vt_batchnorm_stats"], lambda: ops.batchnorm_stats(x, c=C),
            lambda r: [_in("x", x), _out("mean", r[0]), _out("var", r[1]), _out("rstd", r[2])], scratch={9: nb})
    _direct(["vt_batchnorm_act"], lambda: ops.batchnorm_act(x, mean, rstd, gamma, beta, SLOPE, c=C), lambda y: [_in("x", x), _out("y", y, ld=ld, c=C)] + chan)
    dy = _rows(M, C, ld, F32, 7).to(DEV)
    nb = L.load().vt_batchnorm_act_backward_work_bytes(M, C)
    for batch in (True, False):
        ar = _direct(["vt_batchnorm_act_backward"], lambda: ops.batchnorm_act_backward(x, dy, mean, rstd, gamma, beta, SLOPE, batch=batch, c=C),
                     lambda r: [_in("x", x), _in("dy", dy), _out("dx", r[0], ld=ld, c=C), _out("dgamma", r[1]), _out("dbeta", r[2])] + chan, scratch={18: nb})
        assert float(ar.view("dx", dtype, (M, ld))[:, C:].float().abs().max()) == 0          # this operator DEFINES its pad lanes: zero
    y = ops.batchnorm_act(x, mean, rstd, gamma, beta, SLOPE, c=C)
    _direct(["vt_leaky_relu_backward"], lambda: ops.leaky_relu_backward(dy, y, SLOPE), lambda dx: [_in("dy", dy), _in("y", y), _out("dx", dx)])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("with_acc", [False, True], ids=["plain", "acc"])
def test_arena_conv_dgrad_strided(with_acc, dtype):
    ops, _ = _mods()
    g = _strided_geoms()["k4 s2 p1"]
    B, T, H, W, cin, cout = 2, 1, 9, 7, 12, 20
    _, Ho, Wo = g.out_dims(T, H, W)
    w = (torch.randn((cout, cin, 4, 4), generator=_gen(1)) * 0.2).to(DEV)
    dy = torch.randn((B, T, Ho, Wo, 24), generator=_gen(2)).to(dtype).to(DEV)
    acc = torch.randn((B, T, H, W, 16), generator=_gen(3)).to(dtype).to(DEV) if with_acc else None
    ar = _direct(["vt_pack_conv_weight_dgrad"], lambda: ops.pack_conv_weight_dgrad(w, dtype, 24, g), lambda p: [_in("w", w), _out("out", p)])
    wt = ar.view("out", dtype, (4, cin, 4 * 24)).clone()
    ar = _direct(["vt_conv_dgrad"], lambda: ops.conv_dgrad(dy, wt, g, cin=cin, cout=cout, in_hw=(H, W), acc=acc),
                 lambda dx: [_in("dy", dy), _in("wt", wt), _out("dx", dx, ld=16, c=cin)] + ([_in("acc", acc)] if with_acc else []))
    assert float(ar.view("dx", dtype, (B, T, H, W, 16))[..., cin:].float().abs().max()) == 0


def _class_rows(w5, g, cout_p):
    """the blocks [sh * sw, cin, ldw] of vt_pack_conv_weight_dgrad from the host class table: per class its taps in the table's (flipped)
    order, the time taps flipped, Cin / Cout transposed, zeros in the pad channels and past the class's taps"""
    from vidtok_amd.packing import strided_dgrad_classes

    cout, cin, kt = w5.shape[:3]
    ldw = kt * -(-g.kh // g.sh) * -(-g.kw // g.sw) * cout_p
    blocks = []
    for ch, cw in strided_dgrad_classes(g.kh, g.kw, g.sh, g.sw, g.ph, g.pw):
        sub = w5.flip(2)[:, :, :, ch["taps"]][:, :, :, :, cw["taps"]].permute(1, 2, 3, 4, 0)          # [cin, kt, nkh, nkw, cout]
        rows = F.pad(sub, (0, cout_p - cout)).reshape(cin, -1)
        blocks.append(F.pad(rows, (0, ldw - rows.shape[1])))
    return torch.stack(blocks)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pack_conv_weight_dgrad_bits(dtype):
    """the one packer against the host statements, bit for bit: at stride 1 with and without a geometry (pack_rows of
    tests/test_decoder_backward_host.py, inside an arena), under a stride the blocks of the class table"""
    from test_decoder_backward_host import pack_rows

    ops, _ = _mods()
    for shape, cs in (((20, 12, 3, 3, 3), 24), ((20, 12, 1, 4, 4), None)):
        w = torch.randn(shape, generator=_gen(60))
        wd = w.to(DEV)
        kt, kh, kw = shape[2:]
        want = pack_rows(w, cs or ops.pad_channels(20)).to(dtype)
        ar = _direct(["vt_pack_conv_weight_dgrad"], lambda: ops.pack_conv_weight_dgrad(wd, dtype, cs), lambda p: [_in("w", wd), _out("out", p)])
        plain = ar.view("out", dtype, tuple(want.shape)).cpu()
        assert torch.equal(plain, want) and torch.equal(ops.pack_conv_weight_dgrad(wd, dtype, cs).cpu(), want)
        g1 = ops.ConvGeom(kt=kt, kh=kh, kw=kw, pt=kt - 1, ph=1, pw=1, ph_hi=1, pw_hi=1)
        with_geom = ops.pack_conv_weight_dgrad(wd, dtype, cs, g1)
        assert tuple(with_geom.shape) == (1,) + tuple(want.shape) and torch.equal(with_geom[0].cpu(), want)
        assert torch.equal(_class_rows(w, g1, cs or 24).to(dtype), want.unsqueeze(0))                    # the class table says the same
    for gname, shape in (("k4 s2 p1", (20, 12, 1, 4, 4)), ("1x3x3 s21", (20, 12, 1, 3, 3))):
        g = _strided_geoms()[gname]
        w = torch.randn(shape, generator=_gen(61))
        got = ops.pack_conv_weight_dgrad(w.to(DEV), dtype, 24, g)
        want = _class_rows(w, g, 24).to(dtype)
        assert tuple(got.shape) == tuple(want.shape) == (g.sh * g.sw, 12, want.shape[2]) and torch.equal(got.cpu(), want), gname


def test_new_kernels_graph_capture_replays_bit_equal():
    """one linear capture of statistics -> activation -> its backward -> strided data gradient; two replays on new contents are bit-equal
    to eager calls (nothing allocates, synchronises or leaves the caller's stream)"""
    ops, _ = _mods()
    g = _strided_geoms()["k4 s2 p1"]
    c = torch.randn((2, 1, 4, 6, 24), generator=_gen(40)).to(BF16).to(DEV)
    dy = torch.randn(c.shape, generator=_gen(41)).to(DEV)
    gamma, beta = torch.rand(20, device=DEV) + 0.5, torch.randn(20, device=DEV)
    wt = ops.pack_conv_weight_dgrad(torch.randn((20, 12, 4, 4), generator=_gen(42)).to(DEV), BF16, 24, g)

    def run():
        mean, var, rstd = ops.batchnorm_stats(c, c=20)
        y = ops.batchnorm_act(c, mean, rstd, gamma, beta, SLOPE, c=20)
        dc, dg, db = ops.batchnorm_act_backward(c, dy, mean, rstd, gamma, beta, SLOPE, batch=True, c=20)
        dx = ops.conv_dgrad(dc, wt, g, cin=12, cout=20, in_hw=(9, 12))
        return [y, ops.leaky_relu_backward(dy, y, SLOPE), mean, var, dc, dg, db, dx]

    run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    prev = None
    for i in range(2):
        c.copy_(torch.randn(c.shape, generator=_gen(50 + i)).to(BF16))
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        want = run()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got, want)), i
        assert prev is None or not torch.equal(got[0], prev)
        prev = got[0]


# ---- 6. ops.conv_wgrad at the five layer geometries ------------------------------------------------------------------------------------------
LAYERS = [(3, 8, 64, 2, (27, 36)), (64, 64, 128, 2, (13, 18)), (128, 128, 256, 2, (6, 9)), (256, 256, 512, 1, (3, 4)), (512, 512, 1, 1, (2, 3))]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("layer", range(5))
def test_conv_wgrad_layer_geometries(layer, dtype):
    """4 x 4 taps, Cin 3 stored 8, Cout 1: the discriminator's weight gradients on the extents of a (3, ., 27, 36) batch, the gates of the
    existing wgrad tests (1e-5 of fp64 on the stored operands)"""
    ops, _ = _mods()
    cin, ldx, cout, s, (H, W) = LAYERS[layer]
    g = ops.ConvGeom(kh=4, kw=4, sh=s, sw=s, ph=1, pw=1, ph_hi=1, pw_hi=1)
    _, Ho, Wo = g.out_dims(1, H, W)
    x = torch.randn((3, 1, H, W, ldx), generator=_gen(20 + layer)).to(dtype)
    dy = torch.randn((3, 1, Ho, Wo, ops.pad_channels(cout)), generator=_gen(30 + layer)).to(dtype)
    dw, db = ops.conv_wgrad(x.to(DEV), dy.to(DEV), g, cin=cin, cout=cout)
    w = torch.zeros((cout, cin, 4, 4), dtype=torch.float64, requires_grad=True)
    b = torch.zeros((cout,), dtype=torch.float64, requires_grad=True)
    xi = x.double()[:, 0, :, :, :cin].permute(0, 3, 1, 2)
    y = F.conv2d(xi, w, b, stride=s, padding=1)
    (y * dy.double()[:, 0, :, :, :cout].permute(0, 3, 1, 2)).sum().backward()
    ew, eb = rel_err(dw.reshape(w.shape), w.grad), rel_err(db, b.grad)
    print(f"[wgrad] layer {layer} {dtype}: dW {ew:.2e} db {eb:.2e}")
    assert ew <= 1e-5 and eb <= 1e-5, (ew, eb)


# ---- 7. the whole network --------------------------------------------------------------------------------------------------------------------
NET_SHAPES = [(3, 3, 27, 36), (2, 3, 32, 24), (5, 3, 24, 24)]
NET_IDS = ["3x27x36", "2x32x24", "5x24x24"]


@functools.lru_cache(maxsize=None)
def _net():
    return R.seeded()


@functools.lru_cache(maxsize=None)
def _ref(si, train, dtype=torch.float64):
    torch.set_num_threads(16)
    return R.run(_net(), R.make_inputs(NET_SHAPES[si], si), train, dtype, seed=si)


def _ours(train, dtype):
    from vidtok_amd.discriminator import NLayerDiscriminator

    d = NLayerDiscriminator()
    d.load_state_dict(_net().state_dict(), strict=True)
    return d.to(DEV).train(train).set_compute_dtype(dtype)


def _step(d, x, cot, x_grad=True):
    """one forward_with_grad + backward -> (logits, dx or None, {key: grad})"""
    for p in d.parameters():
        p.grad = None
    xx = x.clone().requires_grad_(x_grad)
    y = d.forward_with_grad(xx)
    (y * cot).sum().backward()
    return y.detach(), xx.grad, {k: p.grad for k, p in d.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("si", range(3), ids=NET_IDS)
def test_network_vs_fp64_autograd(si, train, dtype):
    """fp32: logits max|d|/max|ref| <= 1e-4, dx and every parameter gradient relative L2 <= 1e-4.  bf16: the relative L2 distance to fp64
    of the logits, dx and each parameter gradient <= 2 x the distance of torch's own bf16 autograd of the restatement on the CPU.
    Measured on an MI355X (profiles/patchgan.md, "Accuracy"): fp32 logits <= 2.4e-6, dx <= 1.6e-6, parameters <= 1.9e-6; bf16 ours / torch's:
    logits 0.23-1.11 % / 0.23-0.82 %, dx 5.6-8.4 % / 6.3-9.3 %, worst parameter 11.4 % / 12.4 %, largest ratio 1.94 (main.11.bias, one scalar)."""
    ref = _ref(si, train)
    x, cot = R.make_inputs(NET_SHAPES[si], si).to(DEV), ref["cot"].to(DEV)
    d = _ours(train, dtype)
    plain = _ours(train, dtype)(x)
    y, dx, grads = _step(d, x, cot)
    assert y.dtype == F32 and y.shape == ref["logits"].shape and torch.equal(y, plain), "forward_with_grad: the bits of forward"
    assert d.last_dtype == dtype and set(grads) == set(ref["grads"]) and dx.shape == x.shape
    y2, dx2, grads2 = _step(_ours(train, dtype), x, cot)
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and all(torch.equal(grads[k], grads2[k]) for k in grads), "two runs: the same bits"
    # running statistics: one momentum step in train mode, untouched in eval mode
    for k, v in d.named_buffers():
        want = ref["stats"][k]
        if train and dtype == F32:
            assert R.rel_max(v, want) <= 1e-5, (k, R.rel_max(v, want))
        elif train:
            # statistics of bf16-stored convolution outputs cannot sit within 1e-5 of fp64 (measured 2.8e-4 on main.3.running_mean): the
            # bf16 rule of this test instead, against torch's own bf16 pass on the CPU (whose buffers are bf16 as well)
            e, eb = R.rel_l2(v, want), R.rel_l2(_ref(si, train, BF16)["stats"][k], want)
            print(f"[patchgan] {NET_IDS[si]} bf16 {k}: rel L2 ours {e:.3e}, torch bf16 (CPU) {eb:.3e}")
            assert e <= 2 * eb, (k, e, eb)
        else:
            assert torch.equal(v.cpu().double(), _net().state_dict()[k].double()) and torch.equal(want, _net().state_dict()[k].double()), k
    if dtype == F32:
        e = R.rel_max(y, ref["logits"])
        errs = {"dx": R.rel_l2(dx, ref["dx"]), **{k: R.rel_l2(g, ref["grads"][k]) for k, g in grads.items()}}
        print(f"[patchgan] {NET_IDS[si]} train {train} fp32: logits {e:.2e}, dx {errs['dx']:.2e}, worst parameter {max(errs.values()):.2e}")
        assert e <= 1e-4, e
        assert all(v <= 1e-4 for v in errs.values()), errs
    else:
        base = _ref(si, train, torch.bfloat16)
        pairs = {"logits": (y, base["logits"], ref["logits"]), "dx": (dx, base["dx"], ref["dx"]),
                 **{k: (g, base["grads"][k], ref["grads"][k]) for k, g in grads.items()}}
        bad = {}
        for k, (got, b, r) in pairs.items():
            e, eb = R.rel_l2(got, r), R.rel_l2(b, r)
            print(f"[patchgan] {NET_IDS[si]} train {train} bf16 {k}: rel L2 ours {e:.3e}, torch bf16 autograd (CPU) {eb:.3e} (gate 2x = {2 * eb:.3e})")
            if e > 2 * eb:
                bad[k] = (e, eb)
        assert not bad, bad


def test_train_mode_needs_more_than_one_row_per_channel():
    d = _ours(True, F32)
    assert d(torch.zeros((1, 3, 24, 24), device=DEV)).shape == (1, 1, 1, 1)       # 24 -> 12 -> 6 -> 3 -> 2: four rows at the last BatchNorm
    with pytest.raises(ValueError, match="more than 1 value per channel"):        # 16 -> 8 -> 4 -> 2 -> 1: one row, as nn.BatchNorm2d
        d(torch.zeros((1, 3, 16, 16), device=DEV))

def test_selective_gradients_and_wgrad_launches(monkeypatch):
    ops, _ = _mods()
    si = 2
    ref = _ref(si, True)
    x, cot = R.make_inputs(NET_SHAPES[si], si).to(DEV), ref["cot"].to(DEV)
    calls = []
    real = ops.conv_wgrad
    monkeypatch.setattr(ops, "conv_wgrad", lambda x_, dy, g, **kw: calls.append(kw["cout"]) or real(x_, dy, g, **kw))
    d = _ours(True, F32)
    full_y, full_dx, full = _step(d, x, cot)
    assert sorted(calls) == [1, 64, 128, 256, 512]
    # x detached: only parameter gradients, the same bits
    calls.clear()
    y, dx, grads = _step(_ours(True, F32), x, cot, x_grad=False)
    assert dx is None and set(grads) == set(full) and all(torch.equal(grads[k], full[k]) for k in full) and len(calls) == 5
    # every parameter frozen: only x.grad, no weight-gradient launch; x detached as well: the plain value
    calls.clear()
    d = _ours(True, F32).requires_grad_(False)
    y, dx, grads = _step(d, x, cot)
    assert not grads and not calls and torch.equal(dx, full_dx) and torch.equal(y, full_y)
    plain = _ours(True, F32).requires_grad_(False).forward_with_grad(x)
    assert not plain.requires_grad and torch.equal(plain, full_y)
    # one frozen convolution weight: no vt_conv_wgrad launch for it, the other gradients unchanged
    calls.clear()
    d = _ours(True, F32)
    d.main[2].weight.requires_grad_(False)
    y, dx, grads = _step(d, x, cot)
    assert sorted(calls) == [1, 64, 256, 512] and "main.2.weight" not in grads
    assert torch.equal(dx, full_dx) and all(torch.equal(grads[k], full[k]) for k in grads) and set(grads) == set(full) - {"main.2.weight"}


def test_second_backward_fails():
    si = 2
    x = R.make_inputs(NET_SHAPES[si], si).to(DEV).requires_grad_(True)
    y = _ours(True, F32).forward_with_grad(x)
    y.sum().backward(retain_graph=True)
    with pytest.raises(Exception):
        y.sum().backward()


def test_autocast_runs_bf16_kernels():
    si = 2
    ref = _ref(si, True)
    x, cot = R.make_inputs(NET_SHAPES[si], si).to(DEV), ref["cot"].to(DEV)
    y_w, dx_w, _ = _step(_ours(True, BF16), x, cot)
    d = _ours(True, F32)
    xx = x.clone().requires_grad_(True)
    with torch.autocast(device_type="cuda", dtype=BF16):
        y = d.forward_with_grad(xx)
    assert d.last_dtype == BF16 and y.dtype == F32
    (y * cot).sum().backward()                                    # outside the region: the pass keeps its arithmetic
    assert torch.equal(y.detach(), y_w) and torch.equal(xx.grad, dx_w)
    with torch.autocast(device_type="cuda", dtype=torch.float16):
        with pytest.raises(NotImplementedError, match="fp16 has no loss scaling"):
            d.forward_with_grad(xx)


# ---- 8. chained with the decoder's backward, then one discriminator step ---------------------------------------------------------------------
def test_chain_generator_step_then_discriminator_step():
    from util import build_model

    def frames(v):
        return v.permute(0, 2, 1, 3, 4).reshape(-1, v.shape[1], *v.shape[3:])

    vt, _, _ = build_model("vidtok_kl_causal_488_4chn", seed=7, device=DEV, dtype=torch.float32)
    x = (torch.rand(1, 3, 5, 32, 32, generator=_gen(4)) * 2 - 1).to(DEV)
    torch.manual_seed(1)
    z = vt.encode(x)
    disc = _ours(True, F32)
    state = {k: v.clone() for k, v in disc.state_dict().items()}

    def run(two_step):
        disc.load_state_dict(state)
        for p in vt.decoder.parameters():
            p.grad = None
        xh = vt.decode_with_grad(z.detach())
        if two_step:
            leaf = frames(xh).detach().requires_grad_(True)
            (-disc.forward_with_grad(leaf).mean()).backward()
            frames(xh).backward(leaf.grad)
        else:
            (-disc.forward_with_grad(frames(xh)).mean()).backward()          # the reference's non-saturating generator loss
        return {k: p.grad.clone() for k, p in vt.decoder.named_parameters() if p.grad is not None}

    for p in disc.parameters():
        p.requires_grad_(False)
    g1, g2 = run(False), run(True)
    assert g1 and set(g1) == set(g2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    assert all(bool(torch.isfinite(g).all()) for g in g1.values()) and any(bool((g != 0).any()) for g in g1.values())
    assert bool((g1["conv_out.conv.weight"] != 0).any())
    # the discriminator step on detached frames: hinge loss, one optimiser step, and the next forward runs the new weights
    for p in disc.parameters():
        p.requires_grad_(True)
    fake, real = frames(vt.decode_with_grad(z.detach())).detach(), frames(x)
    before = disc(fake)
    opt = torch.optim.SGD(disc.parameters(), lr=0.05)
    opt.zero_grad()
    lr_, lf_ = disc.forward_with_grad(real), disc.forward_with_grad(fake)
    (0.5 * (F.relu(1.0 - lr_).mean() + F.relu(1.0 + lf_).mean())).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in disc.parameters())
    opt.step()
    after = disc(fake)
    assert bool(torch.isfinite(after).all()) and not torch.equal(before, after), "optimizer.step() must reach the packed weights"
