"""Host-side checks of the backward building blocks and of the graph cache's parameter-version tracking (no GPU needed)."""
import ctypes as C
import os
import re

import pytest
import torch

from util import ROOT, build_model


def test_wgrad_desc_matches_header(built_lib):
    from vidtok_amd import lib

    assert built_lib.vt_wgrad_desc_size() == C.sizeof(lib.WgradDesc)
    hdr = open(os.path.join(ROOT, "include", "vidtok_amd.h")).read()
    body = hdr[hdr.index("typedef struct vt_wgrad_desc {") + len("typedef struct vt_wgrad_desc {"):hdr.index("} vt_wgrad_desc;")]
    decl = []
    for stmt in body.split(";"):
        m = re.match(r"\s*(?:const\s+)?(?:void|float|int32_t|int64_t)\s*\*?\s*(.+)$", stmt.strip(), flags=re.S)
        if m:
            decl += [n.strip() for n in m.group(1).split(",")]
    assert decl == [f[0] for f in lib.WgradDesc._fields_]


def _desc(**kw):
    from vidtok_amd import lib

    d = lib.WgradDesc()
    d.B, d.Ti, d.Hi, d.Wi, d.ldx, d.Cin = 1, 5, 8, 8, 128, 128
    d.To, d.Ho, d.Wo, d.lddy, d.Cout = 5, 8, 8, 128, 128
    d.KT, d.KH, d.KW, d.st, d.sh, d.sw = 3, 3, 3, 1, 1, 1
    d.pt, d.ph, d.pw, d.pt_hi, d.ph_hi, d.pw_hi = 2, 1, 1, 0, 1, 1
    d.tmode, d.ups_t, d.ups_s, d.dtype = lib.VT_TPAD_ZERO, 0, 0, lib.VT_BF16
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_conv_wgrad_workspace_and_refusals(built_lib):
    """the workspace holds one fp32 partial tile set per pixel range; invalid descriptors are refused before any device work
    (the pointers below are never dereferenced)"""
    from vidtok_amd import lib

    d = _desc()
    nb = built_lib.vt_conv_wgrad_work_bytes(C.byref(d))
    assert nb >= 128 * 27 * 128 * 4 and nb % 256 == 0
    assert built_lib.vt_conv_wgrad_work_bytes(C.byref(_desc(dtype=lib.VT_F32))) == nb          # the split depends on the shape only
    for bad in (dict(dtype=lib.VT_F16), dict(tmode=lib.VT_TPAD_CACHE), dict(ups_s=2), dict(Cin=129), dict(lddy=64), dict(st=0), dict(Wo=0)):
        assert built_lib.vt_conv_wgrad_work_bytes(C.byref(_desc(**bad))) == -1, bad
    fake = 1 << 20
    d = _desc()
    d.x = d.dy = d.dw = d.work = fake
    d.work_bytes = nb - 1
    assert built_lib.vt_conv_wgrad(C.byref(d), None) == -1 and b"workspace" in built_lib.vt_last_error()
    d = _desc(Ho=9)                   # 9 output rows cannot come from 8 input rows under a same-padded 3x3
    d.x = d.dy = d.dw = d.work = fake
    d.work_bytes = built_lib.vt_conv_wgrad_work_bytes(C.byref(d))
    assert built_lib.vt_conv_wgrad(C.byref(d), None) == -1 and b"extent" in built_lib.vt_last_error()
    d = _desc()
    assert built_lib.vt_conv_wgrad(C.byref(d), None) == -1 and b"null" in built_lib.vt_last_error()


def test_layernorm_backward_refusals(built_lib):
    from vidtok_amd import lib

    assert built_lib.vt_layernorm_act_backward_work_bytes(1000, 513) == -1      # every LayerNorm site has C <= 512
    nb = built_lib.vt_layernorm_act_backward_work_bytes(1000, 512)
    assert nb > 0 and nb % 256 == 0
    fake = C.c_void_p(1 << 20)
    args = lambda **kw: dict(dict(dtype=lib.VT_F32, ld=512, dx_dtype=lib.VT_F32, ldo=512, C_=512, work_bytes=nb), **kw)  # noqa: E731

    def call(a):
        return built_lib.vt_layernorm_act_backward(fake, fake, a["dtype"], a["ld"], fake, a["dx_dtype"], a["ldo"], fake, fake, None, None,
                                                   1000, a["C_"], 1e-6, 1, fake, a["work_bytes"], None)

    for bad in (dict(dtype=lib.VT_F16), dict(dx_dtype=lib.VT_BF16), dict(ld=256), dict(work_bytes=nb - 1), dict(ldo=640)):
        assert call(args(**bad)) == -1, bad


class _Counting:
    def __init__(self):
        self.calls = 0

    def __call__(self, x):
        self.calls += 1
        return x + 1


def test_graph_cache_drops_entries_when_parameter_versions_move():
    """graphs.GraphedCall with a version_fn: a changed fingerprint sends the next call back to the eager first-sight path
    instead of a capture / replay of the old launch sequence (host logic only: the device methods are stubbed)"""
    from vidtok_amd.graphs import GraphedCall

    ver = [0]
    fn = _Counting()
    gc = GraphedCall(fn, version_fn=lambda: ver[0])
    gc._on_device = lambda x: True
    x = torch.zeros(3)
    assert torch.equal(gc(x), x + 1) and gc.entries[((3,), x.dtype, x.device, ())] == "warm"
    ver[0] += 1                                # an in-place update: without the check the next call would capture
    assert torch.equal(gc(x), x + 1) and fn.calls == 2
    assert list(gc.entries.values()) == ["warm"]


def test_engine_parameter_fingerprints_follow_in_place_updates():
    model, _cfg, _sd = build_model("vidtok_kl_causal_488_4chn", seed=3)
    e0, d0 = model._encoder_version(), model._decoder_version()
    with torch.no_grad():
        model.decoder.conv_out.conv.weight.mul_(0.5)
    assert model._decoder_version() != d0 and model._encoder_version() == e0
    opt = torch.optim.SGD(model.encoder.parameters(), lr=0.1)
    for p in model.encoder.parameters():
        p.grad = torch.zeros_like(p)
    opt.step()
    assert model._encoder_version() != e0
    model.invalidate_graphs()                  # the parameter lists are collected afresh (e.g. after .to())
    assert "_graph_params" not in model.__dict__ and model._decoder_version() >= d0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ops_wrappers_refuse_cpu_tensors(dtype):
    from vidtok_amd import lib as L
    from vidtok_amd import ops

    x = torch.zeros((1, 3, 4, 4, 8), dtype=dtype)
    with pytest.raises(L.VtError, match="GPU only"):
        ops.conv_wgrad(x, x, ops.ConvGeom(), cin=8, cout=8)
    with pytest.raises(L.VtError, match="GPU only"):
        ops.layernorm_act_backward(x, x, torch.ones(8), torch.zeros(8), silu=True)


# ---- the harness of the decoder-site tests, checked where there is no GPU ---------------------------------------------------
def test_edge_geometries_are_the_engines_own():
    """the strided / phase geometries of the GPU unit grid are what the engine's modules build"""
    import backward_sites as S
    from vidtok_amd import modules as M

    G = {k: g for k, (g, _) in S.edge_geoms().items()}
    assert G["time-down 3x3x3 st2"] == M.TimeDownsampleResCausal2x(8, 8).conv.geom()
    assert G["3x3x3 s222"] == M.CausalConv3d(8, 8, 3, stride=(2, 2, 2)).geom()
    assert G["1x3x3 s21"] == M.CausalConv3d(8, 8, (1, 3, 3), stride=(1, 2, 1)).geom()
    assert G["up_t 3x3x3"] == M.CausalConv3d(8, 8, 3).geom(1)
    c1 = M.CausalConv1d(8, 8, 3, stride=2)
    assert G["time-down 3x1x1 st2"] == M.ConvGeom(kt=c1.k, st=c1.stride, pt=c1.time_pad)
    assert G["1x3x3"] == M._G3x3 and G["1x1x1"] == M._G1x1
    assert {G[f"phase 2x2 {py}{px}"] for py in (0, 1) for px in (0, 1)} == {site.geom for _py, _px, site in M.Upsample(8, True).parity_sites}


def test_tap_by_tap_wgrad_reference_matches_autograd():
    """backward_sites.ref_wgrad_taps (one fp64 GEMM per tap, what the large sites use) against ref_wgrad (torch autograd through
    conv3d) on every geometry of the unit grid, both time-pad modes, odd and even extents, pad channels in x and dy"""
    import backward_sites as S
    from util import rel_err

    gen = torch.Generator().manual_seed(1)
    for name, (g, tmodes) in S.edge_geoms().items():
        for dims in ((2, 3, 5, 7), (1, 4, 6, 4)):
            x = torch.randn(dims + (8,), generator=gen)
            dy = torch.randn((dims[0],) + g.out_dims(*dims[1:]) + (16,), generator=gen)
            for tmode in tmodes:
                (aw, ab), (bw, bb) = S.ref_wgrad_taps(x, dy, g, 5, 11, tmode), S.ref_wgrad(x, dy, g, 5, 11, tmode)
                assert rel_err(aw, bw) <= 1e-12 and rel_err(ab, bb) <= 1e-12, (name, dims, tmode)


def test_plan_rules_match_the_library(built_lib):
    """backward_sites.wgrad_plan / ln_backward_plan restate the documented split rules; the library's work-byte queries agree on the
    shapes of the GPU grid and on a sweep, so the GPU tests' expectations about ranges and idle workgroups hold for the build at hand"""
    import backward_sites as S

    for M in (21, 32, 2048, 32768, 32256, 16810, 2 * 17 * 256 * 256, 70, 32674):
        for ldx, cout, taps in ((8, 8, 1), (128, 128, 27), (72, 130, 9)):
            d = _desc(B=1, To=1, Ho=1, Wo=M, Ti=1, Hi=1, Wi=M, ldx=ldx, Cin=ldx, Cout=cout, lddy=cout, KT=1, KH=1, KW=taps, pt=0, ph=0,
                      ph_hi=0, pw=taps - 1, pw_hi=0)
            assert built_lib.vt_conv_wgrad_work_bytes(C.byref(d)) == S.wgrad_plan(M, taps * ldx, cout)[2], (M, ldx, cout, taps)
    for M in (1, 3, 4, 5, 33, 4096 * 32, 4096 * 32 + 1, 4096 * 32 + 4097):
        for c in (3, 64, 192, 512):
            assert built_lib.vt_layernorm_act_backward_work_bytes(M, c) == S.ln_backward_plan(M, c)[3]


@pytest.mark.parametrize("key", ["v1_0", "v1_1"])
def test_decoder_site_table_reproduces_whole_graph_gradients(key):
    """The site table and the geometry mapping, before any kernel is involved: for every convolution and LayerNorm site recorded in
    one fp32 autograd pass through oracle.decoder_forward, the fp64 per-site recomputation -- from the site's recorded input and
    output gradient, laid out and padded as the kernel would get them, with the geometry and time-pad mode the engine's modules
    give -- equals the whole-graph weight / bias / gamma / beta gradient and the gradient of the pre-norm rows.  1e-4: fp32 autograd
    against fp64; a wrong site, pad mode, stride or up-sampling is an error of order 1.  Every decoder parameter but the up-samplers'
    mix factors is covered, each by exactly one site."""
    import backward_sites as S
    from util import rel_err
    from vidtok_amd import lib as L

    model, convs, norms, leaves = S.decoder_sites(key)
    assert len(convs) == 65 and len(norms) == 54
    assert all(v.grad is not None for v in leaves.values())
    assert S.compared_parameters(convs, norms) == S.expected_parameters(leaves)
    assert {k for k in leaves if k.endswith(".mix_factor")} == {f"decoder.up_temporal.{i}.upsample.mix_factor" for i in (1, 2)}
    seen = set()
    for s in convs:
        x, dy, g, cin, cout, tmode = S.kernel_conv_operands(model, s, torch.float32)
        assert x.shape[-1] % 8 == 0 and dy.shape[-1] % 8 == 0 and (cin, cout) == tuple(S.weight5(s.dw).shape[1::-1])
        seen.add((g, tmode))
        rw, rb = S.ref_wgrad_taps(x, dy, g, cin, cout, tmode)
        assert rel_err(rw, S.weight5(s.dw)) <= 1e-4, (s.name, g, tmode, rel_err(rw, S.weight5(s.dw)))
        if s.name.endswith(".attn_1.k.conv"):
            # no gradient reaches the key projection's bias (softmax is blind to a shift of every key): both sides are rounding of a
            # sum that cancels, so they are compared on the scale of its terms
            scale = s.dy.abs().sum(dim=(0, 2, 3, 4)).max().item()
            assert rb.abs().max().item() <= 1e-4 * scale and s.db.abs().max().item() <= 1e-4 * scale
        else:
            assert rel_err(rb, s.db) <= 1e-4, (s.name, rel_err(rb, s.db))
    # what the future autograd path relies on: the causal 3-tap convolutions pad two frames in front (zeros under v1.0, the first
    # frame under v1.1), the spatial up-sampler's convolution reads the tensor in front of the up-sampling, the temporal one too
    # where it is nearest (v1.0) and the interpolated tensor where it is trilinear (v1.1)
    tm = L.VT_TPAD_ZERO if key == "v1_0" else L.VT_TPAD_REPLICATE
    by_name = {s.name: S.site_geometry(model, s) for s in convs}
    g, t, _x = by_name["decoder.mid.block_1.conv1.conv"]
    assert (g.kt, g.kh, g.pt, t) == (3, 3, 2, tm)
    g, t, x = by_name["decoder.up.2.upsample.conv"]
    assert g.ups_s == 1 and t == L.VT_TPAD_ZERO and tuple(x.shape[3:]) == (10, 12)
    g, t, x = by_name["decoder.up_temporal.2.upsample.conv.conv"]
    assert (g.ups_t, x.shape[2], t) == ((1, 3, tm) if key == "v1_0" else (0, 6, tm))
    assert len(seen) == (6 if key == "v1_0" else 5)          # 3x3x3, 3x1x1, 1x3x3, 1x1x1, up_s 1x3x3 (+ up_t 3x3x3 where nearest)
    for s in norms:
        y, dn, gamma, beta, c = S.kernel_norm_operands(s, leaves, torch.float32)
        rdx, rg, rb = S.ref_ln(y, dn, gamma, beta, c, s.silu, 1e-6)
        es = (rel_err(rdx, s.dy_pre.permute(0, 2, 3, 4, 1)), rel_err(rg, s.dgamma), rel_err(rb, s.dbeta))
        assert max(es) <= 1e-4, (s.name, s.silu, es)
    assert sum(not s.silu for s in norms) == 1
