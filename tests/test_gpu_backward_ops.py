"""GPU tests of the backward building blocks (vt_conv_wgrad, vt_layernorm_act_backward) against torch autograd on the CPU,
and of the graph cache after an in-place parameter update."""
import pytest
import torch
import torch.nn.functional as F

import backward_sites as S
from backward_sites import ref_ln as _ref_ln
from backward_sites import ref_wgrad as _ref_wgrad
from util import build_model, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


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


# ---- A. every decoder site, operands and geometry taken from the model ------------------------------------------------------
def _err(a, b, scale=None):
    """util.rel_err, or (for a sum that cancels to nothing) max |a - b| over the magnitude `scale` of what was summed"""
    if scale is None:
        return rel_err(a, b)
    return ((a.detach().double().cpu() - b.double()).abs().max() / scale).item()


def _k_bias_scale(site, dy):
    """The bias of the attention's key projection has no gradient: softmax over the keys does not see a shift of all of them, so
    every channel's dy sums to zero over the pixels and what is left in db is rounding of the terms (here 1e-3 of their magnitude at
    most, asserted).  max |b| is then no measure of anything; the error is taken against the largest sum of |dy| over the pixels
    instead -- the scale a relative error of any other bias is taken against, up to its cancellation."""
    if not site.name.endswith(".attn_1.k.conv"):
        return None
    cout = site.dy.shape[1]
    d = dy.double()[..., :cout].reshape(-1, cout)
    scale = d.abs().sum(dim=0).max().item()
    assert d.sum(dim=0).abs().max().item() <= 1e-3 * scale
    return scale


@pytest.mark.parametrize("key,dtype", [("v1_0", torch.float32), ("v1_0", torch.bfloat16), ("v1_1", torch.float32), ("v1_1", torch.bfloat16)])
def test_decoder_sites_match_autograd(key, dtype):
    """vt_conv_wgrad / vt_layernorm_act_backward at every convolution and LayerNorm site of a whole decoder (v1.0: zero front pad;
    v1.1: replicate pad, trilinear up-sampler), on the operands a real backward pass produces (post-SiLU inputs, gradients whose scale
    differs by orders of magnitude from layer to layer, off-centre pre-norm rows) and with the geometry / time-pad mode the engine's
    own modules give.  Reference: fp64, per site, from the same rounded operands; bounds 1e-5 as in the unit grid.
    Measured on an MI355X (worst site of the four runs): see profiles/wgrad_bench.md, "accuracy"."""
    from vidtok_amd import ops

    model, convs, norms, leaves = S.decoder_sites(key)
    assert len(convs) > 0 and len(norms) > 0, "empty site table"
    compared, bad, worst = set(), [], {}

    def note(what, name, e, tol=1e-5):
        print(f"{key} {dtype} {name:48s} {what:7s} {e:.3e}")
        if not e <= tol:
            bad.append((name, what, e))
        if e > worst.get(what, ("", -1.0))[1]:
            worst[what] = (name, e)

    for s in convs:
        x, dy, g, cin, cout, tmode = S.kernel_conv_operands(model, s, dtype)
        rw, rb = S.ref_wgrad_taps(x, dy, g, cin, cout, tmode)
        dw, db = ops.conv_wgrad(x.to(DEV), dy.to(DEV), g, cin=cin, cout=cout, tmode=tmode, bias=s.db is not None)
        assert dw.shape == rw.shape and dw.dtype == torch.float32 and bool(torch.isfinite(dw).all())
        note("dW", s.name, rel_err(dw, rw))
        compared.add(s.name + ".weight")
        if s.db is not None:
            assert bool(torch.isfinite(db).all())
            note("db", s.name, _err(db, rb, _k_bias_scale(s, dy)))
            compared.add(s.name + ".bias")
    for s in norms:
        y, dn, gamma, beta, c = S.kernel_norm_operands(s, leaves, dtype)
        rdx, rg, rb = S.ref_ln(y, dn, gamma, beta, c, s.silu, 1e-6)
        dx, dg, dbt = ops.layernorm_act_backward(y.to(DEV), dn.to(DEV), gamma.to(DEV), beta.to(DEV), silu=s.silu, c=c, dx_dtype=torch.float32)
        assert dx.shape == y.shape and bool(torch.isfinite(dx).all())
        if y.shape[-1] > c:
            assert torch.count_nonzero(dx[..., c:]) == 0
        note("dx", s.name, rel_err(dx[..., :c], rdx))
        note("dgamma", s.name, rel_err(dg, rg))
        note("dbeta", s.name, rel_err(dbt, rb))
        compared |= {s.name + ".weight", s.name + ".bias"}
    print(f"{key} {dtype} worst: {worst}")
    assert compared == S.expected_parameters(leaves), sorted(compared ^ S.expected_parameters(leaves))
    assert not bad, bad


# ---- B. edges of grad.hip ---------------------------------------------------------------------------------------------------
def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _wgrad_poisoned(x, dy, g, cin, cout, tmode, bias=True):
    """vt_conv_wgrad through the C ABI with workspace, dw and db pre-filled with NaN (torch.empty out of the caching allocator hides
    a partial that is read but never written); returns (dw, db, work_bytes)"""
    import ctypes as C

    from vidtok_amd import lib as L
    from vidtok_amd import ops

    lib = L.load()
    d = ops.wgrad_desc(x, dy, g, cin=cin, cout=cout, tmode=tmode)
    nb = lib.vt_conv_wgrad_work_bytes(C.byref(d))
    assert nb > 0 and nb % 4 == 0
    dw, db, work = _nan((cout, cin, g.kt, g.kh, g.kw)), (_nan((cout,)) if bias else None), _nan((nb // 4,))
    d.dw, d.db, d.work, d.work_bytes = dw.data_ptr(), (db.data_ptr() if bias else None), work.data_ptr(), nb
    L.check(lib.vt_conv_wgrad(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "vt_conv_wgrad")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dw).all()) and (db is None or bool(torch.isfinite(db).all())), "an output element was left unwritten or read a NaN partial"
    return dw, db, nb


def _wgrad_case(gname, cin, ldx, cout, lddy, dims, dtype, seed=0):
    """one shape of the edge grid on every time-pad mode of its geometry: poisoned C-ABI call == wrapper call (bits), both on the fp64
    reference"""
    from vidtok_amd import ops

    g, tmodes = S.edge_geoms()[gname]
    B, T, H, W = dims
    gen = torch.Generator().manual_seed(1000 * seed + cin * 7 + cout)
    To, Ho, Wo = g.out_dims(T, H, W)
    assert min(To, Ho, Wo) > 0
    x = (0.5 + torch.randn((B, T, H, W, ldx), generator=gen)).to(dtype)
    dy = torch.randn((B, To, Ho, Wo, lddy), generator=gen).to(dtype)
    for tmode in tmodes:
        rw, rb = S.ref_wgrad_taps(x, dy, g, cin, cout, tmode)
        dw, db, _nb = _wgrad_poisoned(x.to(DEV), dy.to(DEV), g, cin, cout, tmode)
        ew, eb = rel_err(dw, rw), rel_err(db, rb)
        print(f"{gname} cin {cin}/{ldx} cout {cout}/{lddy} {dims} {dtype} tmode {tmode}: dW {ew:.3e} db {eb:.3e}")
        assert ew <= 1e-5 and eb <= 1e-5, (gname, tmode, ew, eb)
        dw2, db2 = ops.conv_wgrad(x.to(DEV), dy.to(DEV), g, cin=cin, cout=cout, tmode=tmode)
        assert torch.equal(dw, dw2) and torch.equal(db, db2)


# (geometry, cin, stored cin, cout, (B, T, H, W)): odd extents (the last strided window ends inside the input) and even ones (it
# uses the high pad); C = 128 with both up-samplings folded, on odd extents
EDGE_CASES = [("downsample 3x3 s2", 128, 128, 128, (2, 3, 7, 9)), ("downsample 3x3 s2", 8, 8, 8, (1, 2, 8, 6)),
              ("time-down 3x3x3 st2", 128, 128, 128, (1, 5, 5, 7)), ("time-down 3x3x3 st2", 5, 8, 8, (2, 4, 5, 3)),
              ("time-down 3x1x1 st2", 128, 128, 128, (2, 7, 5, 3)), ("time-down 3x1x1 st2", 8, 8, 8, (1, 6, 3, 5)),
              ("3x3x3 s222", 128, 128, 64, (1, 5, 7, 9)), ("3x3x3 s222", 8, 8, 8, (2, 4, 6, 8)),
              ("1x3x3 s21", 128, 128, 64, (1, 2, 7, 9)), ("1x3x3 s21", 8, 8, 8, (2, 3, 8, 6)),
              ("centred 3x3x3", 128, 128, 128, (1, 3, 5, 7)), ("centred 3x1x1", 8, 8, 8, (2, 5, 3, 3)),
              ("phase 2x2 00", 128, 128, 128, (1, 2, 5, 7)), ("phase 2x2 01", 128, 128, 128, (1, 2, 5, 7)),
              ("phase 2x2 10", 128, 128, 128, (1, 2, 5, 7)), ("phase 2x2 11", 128, 128, 128, (1, 2, 5, 7)),
              ("up_t 3x3x3", 8, 8, 8, (2, 3, 5, 7)), ("up_t 3x3x3", 128, 128, 128, (1, 3, 5, 7)),
              ("up_s 1x3x3", 128, 128, 128, (1, 3, 5, 7)), ("up_t up_s 3x3x3", 128, 128, 128, (1, 3, 5, 3))]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("gname,cin,ldx,cout,dims", EDGE_CASES)
def test_conv_wgrad_strides_centred_pads_phases_and_folded_upsampling(gname, cin, ldx, cout, dims, dtype):
    from vidtok_amd import ops

    _wgrad_case(gname, cin, ldx, cout, ops.pad_channels(cout), dims, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ldx", [8, 72, 136])
@pytest.mark.parametrize("cout", [96, 130])
def test_conv_wgrad_partial_tiles_on_both_axes(cout, ldx, dtype):
    """Cout and K = 9 x ldx both end inside a 64-wide tile; fewer channels in use than stored (cin < ldx), dy rows wider than Cout"""
    lddy = {96: 104, 130: 136}[cout]
    assert (9 * ldx) % 64 and cout % 64 and lddy > cout
    _wgrad_case("1x3x3", ldx - 3, ldx, cout, lddy, (2, 3, 5, 7), dtype, seed=1)


# (B, To, Ho, Wo), ranges expected.  K = 8 and Cout = 8 make one tile, so the range count is min(stages / 8, 64) before the recount
PLAN_CASES = [((1, 1, 3, 7), 1),        # M = 21 < 32: one partial stage
              ((1, 2, 4, 4), 1),        # M = 32: one full stage
              ((2, 4, 16, 16), 8),      # M = 2048 = 8 ranges of 256 pixels exactly
              ((2, 4, 64, 64), 64),     # 1024 stages: the 64-range cap, every range full
              ((2, 4, 64, 63), 63),     # 1008 stages dealt out 16 at a time: 63 ranges, not the 64 first planned
              ((2, 5, 41, 41), 59)]     # 526 stages, 9 per range: 59 ranges, the last one ending 10 pixels into its fourth stage


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dims,ranges", PLAN_CASES)
def test_conv_wgrad_range_plan_edges(dims, ranges, dtype):
    """the split of the pixel axis at its edges; the expected plan comes from the documented rule (backward_sites.wgrad_plan) and
    vt_conv_wgrad_work_bytes has to agree with it, so a change of the rule cannot leave a range unwritten unnoticed -- and the
    NaN-poisoned workspace shows any partial that is read without having been written"""
    g, _ = S.edge_geoms()["1x1x1"]
    M = dims[0] * dims[1] * dims[2] * dims[3]
    ns, chunk, nbytes = S.wgrad_plan(M, 8, 8)
    assert ns == ranges and chunk % 32 == 0 and (ns - 1) * chunk < M <= ns * chunk
    gen = torch.Generator().manual_seed(M)
    x = (0.5 + torch.randn(dims + (8,), generator=gen)).to(dtype)
    dy = torch.randn(dims + (8,), generator=gen).to(dtype)
    dw, db, nb = _wgrad_poisoned(x.to(DEV), dy.to(DEV), g, 8, 8, 0)
    assert nb == nbytes, (nb, nbytes)
    rw, rb = S.ref_wgrad_taps(x, dy, g, 8, 8, 0)
    assert rel_err(dw, rw) <= 1e-5 and rel_err(db, rb) <= 1e-5, (rel_err(dw, rw), rel_err(db, rb))


@pytest.mark.parametrize("dims,cin,cout,gname", [((2, 17, 31, 31), 128, 128, "centred 3x3x3"), ((1, 2, 5, 7), 128, 130, "1x3x3")])
def test_conv_wgrad_plan_of_multi_tile_shapes_and_poisoned_buffers(dims, cin, cout, gname):
    """a multi-range and a single-range shape with several tiles: work bytes by the rule, every output finite and correct out of
    NaN-filled buffers"""
    from vidtok_amd import ops

    g, _ = S.edge_geoms()[gname]
    M = dims[0] * dims[1] * dims[2] * dims[3]
    ns, _chunk, nbytes = S.wgrad_plan(M, g.kt * g.kh * g.kw * cin, cout)
    assert (ns > 1) == (M > 1000)
    gen = torch.Generator().manual_seed(M)
    x = torch.randn(dims + (cin,), generator=gen).to(torch.bfloat16)
    dy = torch.randn(dims + (ops.pad_channels(cout),), generator=gen).to(torch.bfloat16)
    dw, db, nb = _wgrad_poisoned(x.to(DEV), dy.to(DEV), g, cin, cout, 0)
    assert nb == nbytes, (nb, nbytes)
    rw, rb = S.ref_wgrad_taps(x, dy, g, cin, cout, 0)
    assert rel_err(dw, rw) <= 1e-5 and rel_err(db, rb) <= 1e-5, (rel_err(dw, rw), rel_err(db, rb))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv_wgrad_long_reduction_off_centre(dtype):
    """fine-tuning scale: 1x1x1, 8 -> 8 channels over M = 2 x 17 x 256 x 256 pixels (64 ranges of 34 816), operands not centred
    (x = SiLU(randn), dy = randn + 0.25), so db and the thin dW are long sums of same-signed terms.  fp64 reference: one GEMM.
    Measured on an MI355X: see profiles/wgrad_bench.md, "accuracy"."""
    g, _ = S.edge_geoms()["1x1x1"]
    dims = (2, 17, 256, 256)
    M = 2 * 17 * 256 * 256
    assert S.wgrad_plan(M, 8, 8)[:2] == (64, 34816)
    gen = torch.Generator().manual_seed(23)
    x = F.silu(torch.randn(dims + (8,), generator=gen)).to(dtype)
    dy = (torch.randn(dims + (8,), generator=gen) + 0.25).to(dtype)
    dw, db, _nb = _wgrad_poisoned(x.to(DEV), dy.to(DEV), g, 8, 8, 0)
    xd, dyd = x.double().reshape(M, 8), dy.double().reshape(M, 8)
    rw, rb = (dyd.t() @ xd).reshape(8, 8, 1, 1, 1), dyd.sum(dim=0)
    ew, eb = rel_err(dw, rw), rel_err(db, rb)
    print(f"long reduction {dtype}: dW {ew:.3e} db {eb:.3e}")
    assert ew <= 1e-5 and eb <= 1e-5, (ew, eb)


def test_conv_wgrad_same_bits_without_bias_on_a_side_stream_and_from_an_offset_view():
    """several tiles on both axes (Cout 130, K = 9 x 72) and several ranges: dW does not depend on whether db is asked for, on the
    stream, or on where in its storage an operand starts"""
    from vidtok_amd import ops

    g, _ = S.edge_geoms()["1x3x3"]
    gen = torch.Generator().manual_seed(29)
    x = torch.randn((2, 9, 15, 13, 72), generator=gen).to(DEV, torch.bfloat16)
    dy = torch.randn((2, 9, 15, 13, 136), generator=gen).to(DEV, torch.bfloat16)
    assert S.wgrad_plan(2 * 9 * 15 * 13, 9 * 72, 130)[0] > 1
    dw, db = ops.conv_wgrad(x, dy, g, cin=70, cout=130)
    dw0, none = ops.conv_wgrad(x, dy, g, cin=70, cout=130, bias=False)
    assert none is None and torch.equal(dw, dw0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dw1, db1 = ops.conv_wgrad(x, dy, g, cin=70, cout=130)
    side.synchronize()
    assert torch.equal(dw, dw1) and torch.equal(db, db1)
    xo, dyo = torch.empty(x.numel() + 8, dtype=x.dtype, device=DEV), torch.empty(dy.numel() + 24, dtype=dy.dtype, device=DEV)
    xv, dyv = xo[8:].view(x.shape), dyo[24:].view(dy.shape)
    xv.copy_(x)
    dyv.copy_(dy)
    assert xv.storage_offset() == 8 and dyv.storage_offset() == 24 and xv.is_contiguous()
    dw2, db2 = ops.conv_wgrad(xv, dyv, g, cin=70, cout=130)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    rw, rb = S.ref_wgrad_taps(x, dy, g, 70, 130, 0)
    assert rel_err(dw, rw) <= 1e-5 and rel_err(db, rb) <= 1e-5


def _ln_poisoned(y, dn, gamma, beta, c, silu, dx_dtype, eps=1e-6):
    """vt_layernorm_act_backward through the C ABI with NaN-filled workspace and outputs; returns (dx, dgamma, dbeta, work bytes)"""
    import ctypes as C

    from vidtok_amd import lib as L

    lib = L.load()
    dt = {torch.float32: L.VT_F32, torch.bfloat16: L.VT_BF16}
    ld = y.shape[-1]
    M = y.numel() // ld
    nb = lib.vt_layernorm_act_backward_work_bytes(M, c)
    assert nb > 0 and nb % 4 == 0
    dx, dg, dbt, work = _nan(y.shape, dx_dtype), _nan((c,)), _nan((c,)), _nan((nb // 4,))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    L.check(lib.vt_layernorm_act_backward(p(y), p(dn), dt[y.dtype], ld, p(dx), dt[dx_dtype], ld, p(gamma), p(beta), p(dg), p(dbt), M, c, eps,
                                          int(silu), p(work), nb, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "vt_layernorm_act_backward")
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in (dx, dg, dbt)), "an output element was left unwritten or read a NaN partial"
    return dx, dg, dbt, nb


def _ln_check(y, dn, gamma, beta, c, silu, tag):
    """fp32 dx, dgamma, dbeta on the fp64 reference (1e-5); for bf16 rows also: the bf16 dx is the fp32 dx of the same call rounded to
    nearest-even, bit for bit"""
    rdx, rg, rb = _ref_ln(y, dn, gamma, beta, c, silu, 1e-6)
    yd, dnd, gd, bd = y.to(DEV), dn.to(DEV), gamma.to(DEV), beta.to(DEV)
    dx, dg, dbt, nb = _ln_poisoned(yd, dnd, gd, bd, c, silu, torch.float32)
    es = (rel_err(dx[..., :c], rdx), rel_err(dg, rg), rel_err(dbt, rb))
    print(f"{tag}: dx {es[0]:.3e} dgamma {es[1]:.3e} dbeta {es[2]:.3e}")
    assert max(es) <= 1e-5, (tag, es)
    if y.shape[-1] > c:
        assert torch.count_nonzero(dx[..., c:]) == 0
    if y.dtype == torch.bfloat16:
        dxh, dgh, dbh, _ = _ln_poisoned(yd, dnd, gd, bd, c, silu, torch.bfloat16)
        assert torch.equal(dxh, dx.to(torch.bfloat16)) and torch.equal(dgh, dg) and torch.equal(dbh, dbt)
    return nb


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("c", [64, 96, 192, 320, 384, 448, 512, 3, 4, 65])
def test_layernorm_act_backward_every_lane_layout(c, silu, dtype):
    """every (channels per lane, slots in use) pair of the kernel: C = 192 runs the 4-slot form with 3 in use, C = 320 / 384 / 448 the
    8-slot form with 5 / 6 / 7, C = 65 and 96 end inside a slot; ld = pad_channels(C)"""
    from vidtok_amd import ops

    ld = ops.pad_channels(c)
    gen = torch.Generator().manual_seed(3 * c + silu)
    shape = (2, 3, 5, 7, ld)
    y = (0.5 + 2.0 * torch.randn(shape, generator=gen)).to(dtype)
    dn = torch.randn(shape, generator=gen).to(dtype)
    gamma, beta = 1.0 + 0.1 * torch.randn((c,), generator=gen), 0.1 * torch.randn((c,), generator=gen)
    _ln_check(y, dn, gamma, beta, c, silu, f"C {c} silu {silu} {dtype}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M", [1, 3, 4, 5, 33, 4096 * 32, 4096 * 32 + 1, 4096 * 32 + 4097])
def test_layernorm_act_backward_row_counts(M, dtype):
    """fewer rows than waves, the 4096-workgroup cap, and past it: rows dealt out 33 / 34 to a workgroup, which leaves trailing
    workgroups without a row -- their partials must be written (as zeros), which the NaN-filled workspace checks"""
    groups, rows, idle, nbytes = S.ln_backward_plan(M, 64)
    assert (groups, rows, idle) == {1: (1, 1, 0), 3: (1, 3, 0), 4: (1, 4, 0), 5: (1, 5, 0), 33: (2, 17, 0), 4096 * 32: (4096, 32, 0),
                                    4096 * 32 + 1: (4096, 33, 124), 4096 * 32 + 4097: (4096, 34, 120)}[M]
    gen = torch.Generator().manual_seed(M)
    y = (0.5 + 2.0 * torch.randn((M, 64), generator=gen)).to(dtype)
    dn = torch.randn((M, 64), generator=gen).to(dtype)
    gamma, beta = 1.0 + 0.1 * torch.randn((64,), generator=gen), 0.1 * torch.randn((64,), generator=gen)
    assert _ln_check(y, dn, gamma, beta, 64, True, f"M {M} {dtype}") == nbytes


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("c", [128, 512])
@pytest.mark.parametrize("mean,std", [(8.0, 1.0), (30.0, 1.0), (-8.0, 0.25)])
def test_layernorm_act_backward_off_centre_rows(mean, std, c, dtype):
    """rows far from zero relative to their spread (what a residual stream looks like deep in the decoder): the statistics are
    recomputed in two passes, so the variance must not lose its digits to the mean"""
    gen = torch.Generator().manual_seed(int(mean * 10) + c)
    y = (mean + std * torch.randn((2, 3, 5, 7, c), generator=gen)).to(dtype)
    dn = torch.randn(y.shape, generator=gen).to(dtype)
    gamma, beta = 1.0 + 0.1 * torch.randn((c,), generator=gen), 0.1 * torch.randn((c,), generator=gen)
    for silu in (True, False):
        _ln_check(y, dn, gamma, beta, c, silu, f"mean {mean} std {std} C {c} silu {silu} {dtype}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("c", [128, 192])
def test_layernorm_act_backward_constant_rows(c, dtype):
    """rows of variance exactly 0 (every third row one repeated value, bf16-exact) among ordinary ones: x-hat is 0, rstd = eps^-1/2,
    and dx = rstd (dh - mean(dh)) is a thousand times the other rows' -- finite, and on the reference.  C = 192: the row mean has to be
    sum / C, not sum * fl(1 / C) (one ulp off on a row of 30.0, which rstd turned into an x-hat of 1.9e-3: dx was 7.2e-4 off before
    that was fixed in grad.hip, 1.1e-7 after)"""
    gen = torch.Generator().manual_seed(c)
    y = 0.5 + 2.0 * torch.randn((70, c), generator=gen)
    y[::3] = torch.tensor([0.0, 1.0, -8.0, 30.0, 0.5] * 5)[:y[::3].shape[0], None]
    y = y.to(dtype)
    assert bool((y[::3].float().var(dim=1) == 0).all())
    dn = torch.randn(y.shape, generator=gen).to(dtype)
    gamma, beta = 1.0 + 0.1 * torch.randn((c,), generator=gen), 0.1 * torch.randn((c,), generator=gen)
    for silu in (True, False):
        _ln_check(y, dn, gamma, beta, c, silu, f"constant rows C {c} silu {silu} {dtype}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_layernorm_act_backward_saturated_silu(dtype):
    """gamma = +-60 drives |u| = |gamma x-hat + beta| past 90 on many lanes, where exp(-u) overflows to inf in fp32 (u < -88.7) or
    underflows: SiLU'(u) must come out as 0 and 1, not NaN"""
    c = 128
    gen = torch.Generator().manual_seed(41)
    y = (0.5 + 2.0 * torch.randn((64, c), generator=gen)).to(dtype)
    dn = torch.randn(y.shape, generator=gen).to(dtype)
    gamma = 60.0 * torch.where(torch.arange(c) % 2 == 0, 1.0, -1.0) * (1.0 + 0.1 * torch.randn((c,), generator=gen))
    beta = 0.1 * torch.randn((c,), generator=gen)
    u = F.layer_norm(y.float(), (c,), gamma, beta, 1e-6)
    assert u.max() > 90 and u.min() < -90
    _ln_check(y, dn, gamma, beta, c, True, f"saturated SiLU {dtype}")


# ---- both ops under graph capture -------------------------------------------------------------------------------------------
def _capture_and_replay(run, refill):
    """warm-up call, one linear capture, three replays with the operand contents changed in place between them; every replay is
    bit-equal to an eager call on the same contents"""
    run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for i in range(3):
        refill(i)
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        want = run()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got, want)), i
        if i:
            assert not torch.equal(got[0], prev)         # the replay saw the new contents
        prev = got[0]


def test_conv_wgrad_graph_capture_replays_bit_equal():
    from vidtok_amd import lib as L
    from vidtok_amd import ops

    g, _ = S.edge_geoms()["up_t 3x3x3"]
    gen = torch.Generator().manual_seed(31)
    x = torch.randn((2, 5, 9, 11, 128), generator=gen).to(DEV, torch.bfloat16)
    dy = torch.randn((2, 10, 9, 11, 128), generator=gen).to(DEV, torch.bfloat16)
    assert S.wgrad_plan(2 * 10 * 9 * 11, 27 * 128, 128)[0] > 1

    def refill(i):
        x.copy_(torch.randn(x.shape, generator=gen).to(x.dtype))
        dy.copy_(torch.randn(dy.shape, generator=gen).to(dy.dtype))

    _capture_and_replay(lambda: ops.conv_wgrad(x, dy, g, cin=128, cout=128, tmode=L.VT_TPAD_REPLICATE), refill)
    rw, rb = S.ref_wgrad_taps(x, dy, g, 128, 128, L.VT_TPAD_REPLICATE)
    dw, db = ops.conv_wgrad(x, dy, g, cin=128, cout=128, tmode=L.VT_TPAD_REPLICATE)
    assert rel_err(dw, rw) <= 1e-5 and rel_err(db, rb) <= 1e-5


def test_layernorm_act_backward_graph_capture_replays_bit_equal():
    from vidtok_amd import ops

    c = 192
    gen = torch.Generator().manual_seed(37)
    y = (0.5 + 2.0 * torch.randn((2, 3, 9, 11, c), generator=gen)).to(DEV, torch.bfloat16)
    dn = torch.randn(y.shape, generator=gen).to(DEV, torch.bfloat16)
    gamma, beta = (1.0 + 0.1 * torch.randn((c,), generator=gen)).to(DEV), (0.1 * torch.randn((c,), generator=gen)).to(DEV)

    def refill(i):
        y.copy_((1.0 + torch.randn(y.shape, generator=gen)).to(y.dtype))
        dn.copy_(torch.randn(dn.shape, generator=gen).to(dn.dtype))
        gamma.copy_(1.0 + 0.1 * torch.randn((c,), generator=gen))

    _capture_and_replay(lambda: ops.layernorm_act_backward(y, dn, gamma, beta, silu=True, c=c), refill)
    rdx, rg, rb = _ref_ln(y, dn, gamma, beta, c, True, 1e-6)
    dx, dg, dbt = ops.layernorm_act_backward(y, dn, gamma, beta, silu=True, c=c, dx_dtype=torch.float32)
    assert rel_err(dx, rdx) <= 1e-5 and rel_err(dg, rg) <= 1e-5 and rel_err(dbt, rb) <= 1e-5
