"""Differentiable decode, the part that needs no GPU: the C surface, what is refused, and the MATH the data-gradient kernels implement
restated in torch -- the transposed / tap-flipped pack fed to a forward convolution with mirrored pads plus the folds equals
autograd's input gradient in fp64 on every stride-1 geometry of backward_sites parts A and B; the adjoint of the v1.1 first-chunk
interpolation equals autograd through the oracle's time_upsample."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import backward_sites as S  # noqa: E402
from util import build_model  # noqa: E402

NEW_SYMBOLS = ["vt_dgrad_desc_size", "vt_pack_conv_weight_dgrad", "vt_conv_dgrad_work_bytes", "vt_conv_dgrad", "vt_grad_fold", "vt_softmax_rows_backward",
               "vt_transpose_batched", "vt_upsample_mix", "vt_upsample_mix_backward_work_bytes", "vt_upsample_mix_backward", "vt_time_lerp2x_backward",
               "vt_grad_ncthw_to_ndhwc", "vt_grad_add"]


def test_c_surface():
    from vidtok_amd import lib as L

    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert lib.vt_dgrad_desc_size() == C.sizeof(L.DgradDesc)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vidtok_amd.h")).read()
    body = header[header.index("typedef struct vt_dgrad_desc {"):header.index("} vt_dgrad_desc;")]
    fields = [f.strip().lstrip("*") for line in body.splitlines()[1:] for f in line.split("/*")[0].rstrip("; ").split(" ", 1)[-1].replace("void*", "").replace("void *", "").split(",") if f.strip()]
    fields = [f.split()[-1].lstrip("*") for f in fields]
    assert fields == [n for n, _ in L.DgradDesc._fields_], fields
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name


def test_strides_the_library_serves_and_refuses():
    """vt_conv_dgrad serves st = 1 with sh, sw in {1, 2} (tests/test_patchgan_host.py::test_conv_dgrad_domain has the strided side); a
    time stride and stride 3 are refused with a message, by the size query and by the launch"""
    from vidtok_amd import lib as L

    d = L.DgradDesc()
    d.B, d.Ti, d.Hi, d.Wi, d.lddx, d.Cin = 1, 1, 8, 8, 8, 8
    d.To, d.Ho, d.Wo, d.lddy, d.Cout = 1, 4, 4, 8, 8
    d.KT, d.KH, d.KW, d.st, d.sh, d.sw = 1, 3, 3, 1, 2, 2
    d.ph_hi = d.pw_hi = 1
    d.ldw, d.dtype, d.dx_dtype = 72, L.VT_F32, L.VT_F32
    lib = L.load()
    assert lib.vt_conv_dgrad_work_bytes(C.byref(d)) == 4 * (1 * 1 * 4 * 4 * 8 * 4)         # four classes of 4 x 4 pixels, 512 bytes each
    for st, sh in ((2, 2), (1, 3)):
        d.st, d.sh = st, sh
        assert lib.vt_conv_dgrad_work_bytes(C.byref(d)) == -1 and b"stride" in lib.vt_last_error()
        assert lib.vt_conv_dgrad(C.byref(d), None) != 0 and b"stride" in lib.vt_last_error()
    d.st = d.sh = d.sw = 1                # the same descriptor at stride 1 with matching extents is a plain launch: no workspace
    d.Ho = d.Wo = 7
    assert lib.vt_conv_dgrad_work_bytes(C.byref(d)) == 0
    d.dx_dtype, d.dtype = L.VT_BF16, L.VT_BF16      # a bf16 dx is rounded from an fp32 workspace
    assert lib.vt_conv_dgrad_work_bytes(C.byref(d)) == 1 * 1 * 8 * 8 * 8 * 4
    d.dtype = L.VT_F16
    assert lib.vt_conv_dgrad_work_bytes(C.byref(d)) == -1


def test_ops_raise_on_cpu_tensors():
    from vidtok_amd import lib as L
    from vidtok_amd import ops

    t, f = torch.zeros((1, 2, 4, 4, 8)), torch.zeros((1,))
    calls = [lambda: ops.conv_dgrad(t, torch.zeros((8, 8)), ops.ConvGeom(), cin=8, cout=8),
             lambda: ops.pack_conv_weight_dgrad(torch.zeros((8, 8, 1, 1, 1)), torch.float32),
             lambda: ops.grad_fold(t, ups_t=1),
             lambda: ops.softmax_rows_backward(torch.zeros((2, 4, 8)), torch.zeros((2, 4, 8)), 1.0),
             lambda: ops.transpose_batched(torch.zeros((2, 4, 8))),
             lambda: ops.upsample_mix(t, t, f),
             lambda: ops.upsample_mix_backward(t, t, t, f),
             lambda: ops.time_lerp2x_backward(t, 0, 1, torch.zeros((1, 1, 4, 4, 8)), 0),
             lambda: ops.grad_ncthw_to_ndhwc(torch.zeros((1, 3, 2, 4, 4)), torch.float32),
             lambda: ops.grad_add(t, t)]
    for c in calls:
        with pytest.raises(L.VtError, match="GPU only"):
            c()


Z = torch.zeros((1, 4, 3, 4, 4))


@pytest.mark.parametrize("what", ["groupnorm", "noncausal", "tiling", "fp16", "bf16x3", "give_pre_end", "tanh_out", "autocast fp16"])
def test_refused_configurations(what):
    name, ov, dtype = "vidtok_kl_causal_488_4chn", None, torch.float32
    if what == "groupnorm":
        ov = {"norm_type": "groupnorm"}
    elif what == "noncausal":
        name = "vidtok_kl_noncausal_488_4chn"
    elif what == "tiling":
        name = "vidtok_v1_1/vidtok_kl_causal_488_4chn_v1_1"
    elif what in ("fp16", "bf16x3"):
        dtype = {"fp16": torch.float16, "bf16x3": "bf16x3"}[what]
    model, _cfg, _sd = build_model(name, dtype=dtype, overrides=ov)
    if what == "tiling":
        model.use_tiling = True
    if what in ("give_pre_end", "tanh_out"):
        setattr(model.decoder, what, True)
    if what == "autocast fp16":
        with torch.autocast("cpu", dtype=torch.float16), pytest.raises(NotImplementedError, match="fp16"):
            model.decode_with_grad(Z)
        return
    with pytest.raises(NotImplementedError, match="decode_with_grad"):
        model.decode_with_grad(Z)


def test_decode_stays_under_no_grad():
    """decode / forward / encode keep their no_grad contract: whatever the decoder computes, the result carries no graph"""
    model, _cfg, _sd = build_model("vidtok_kl_causal_488_4chn")
    w = torch.ones((), requires_grad=True)
    model._run_decoder = lambda z: z * w
    out = model.decode(Z.clone().requires_grad_(True))
    assert out.requires_grad is False
    assert not hasattr(torch.nn.Module, "decode_with_grad") and callable(model.decode_with_grad)


# ---- the math of vt_pack_conv_weight_dgrad + vt_conv + vt_grad_fold, restated ------------------------------------------------------
def pack_rows(w5, cout_p):
    """[Cin, taps * cout_p]: taps flipped, Cin / Cout transposed, pad channels zero (vt_pack_conv_weight_dgrad)"""
    cout, cin = w5.shape[:2]
    r = w5.flip(2, 3, 4).permute(1, 2, 3, 4, 0)                      # [cin, kt, kh, kw, cout]
    return F.pad(r, (0, cout_p - cout)).reshape(cin, -1)


def dgrad_by_forward_conv(dy, w5, g, tmode, Ti, Hi, Wi, cout_p):
    """dx NCTHW [B, cin, Ti, Hi, Wi] the way vt_conv_dgrad computes it: a forward convolution over dy (stored channels, zero weights on the
    pad lanes) with mirrored pads, then the folds"""
    from vidtok_amd import lib as L

    cout, cin = w5.shape[:2]
    rows = pack_rows(w5, cout_p)
    wt = rows.view(cin, g.kt, g.kh, g.kw, cout_p).permute(0, 4, 1, 2, 3)              # a forward weight [cin, cout_p, kt, kh, kw]
    Tv, Hv, Wv = Ti << g.ups_t, Hi << g.ups_s, Wi << g.ups_s
    rep = g.pt if tmode == L.VT_TPAD_REPLICATE else 0
    B, _, To, Ho, Wo = dy.shape
    ft = g.kt - 1 if rep else g.kt - 1 - g.pt
    fh, fw = g.kh - 1 - g.ph, g.kw - 1 - g.pw
    bt, bh, bw = (rep + Tv) - (To + ft - g.kt + 1), Hv - (Ho + fh - g.kh + 1), Wv - (Wo + fw - g.kw + 1)
    assert (bt, bh, bw) == (g.kt - 1 - g.pt_hi if not rep else bt, g.kh - 1 - g.ph_hi, g.kw - 1 - g.pw_hi) and min(bt, bh, bw) >= 0
    dyp = F.pad(dy, (0, 0, 0, 0, 0, 0, 0, cout_p - cout), value=3.0)                   # garbage on the pad lanes
    d = F.conv3d(F.pad(dyp, (fw, bw, fh, bh, ft, bt)), wt)
    assert tuple(d.shape) == (B, cin, rep + Tv, Hv, Wv)
    if rep:
        d = torch.cat([d[:, :, :rep + 1].sum(dim=2, keepdim=True), d[:, :, rep + 1:]], dim=2)
    if g.ups_t:
        d = d[:, :, 0::2] + d[:, :, 1::2]
    if g.ups_s:
        d = (d[..., 0::2, 0::2] + d[..., 0::2, 1::2]) + (d[..., 1::2, 0::2] + d[..., 1::2, 1::2])
    return d


def autograd_dx(dy, w5, g, tmode, B, cin, Ti, Hi, Wi):
    x = torch.zeros((B, Ti, Hi, Wi, cin), dtype=torch.float64, requires_grad=True)
    y = F.conv3d(S.virtual_input(x, g, tmode), w5)
    assert y.shape == dy.shape, (y.shape, dy.shape)
    (y * dy).sum().backward()
    return x.grad.permute(0, 4, 1, 2, 3)


def stride1_geometries():
    """every (geometry, time-pad mode) of the decoder sites of both models (part A) and of the stride-1 edge grid (part B), each under
    zero and replicate"""
    from vidtok_amd import lib as L

    out = {}
    for key in ("v1_0", "v1_1"):
        model, convs, _n, _l = S.decoder_sites(key)
        for s in convs:
            g, tmode, _x = S.site_geometry(model, s)
            out[(g, tmode)] = "site " + s.name
    n_sites = len(out)
    for name, (g, _tm) in S.edge_geoms().items():
        if (g.st, g.sh, g.sw) == (1, 1, 1):
            out.setdefault((g, L.VT_TPAD_ZERO), name)
    for (g, _tm), name in list(out.items()):
        for tmode in (L.VT_TPAD_ZERO, L.VT_TPAD_REPLICATE):
            out.setdefault((g, tmode), name)
    assert n_sites >= 6
    return out


def test_pack_mode_math_equals_autograd():
    gen = torch.Generator().manual_seed(0)
    B, Ti, Hi, Wi, cin, cout, cout_p = 2, 3, 4, 5, 3, 5, 8
    geoms = stride1_geometries()
    assert len(geoms) >= 20
    for (g, tmode), name in geoms.items():
        To, Ho, Wo = g.out_dims(Ti, Hi, Wi)
        w5 = torch.randn((cout, cin, g.kt, g.kh, g.kw), generator=gen, dtype=torch.float64)
        dy = torch.randn((B, cout, To, Ho, Wo), generator=gen, dtype=torch.float64)
        got = dgrad_by_forward_conv(dy, w5, g, tmode, Ti, Hi, Wi, cout_p)
        ref = autograd_dx(dy, w5, g, tmode, B, cin, Ti, Hi, Wi)
        err = ((got - ref).abs().max() / ref.abs().max()).item()
        assert err <= 1e-12, (name, g, tmode, err)
    rows = pack_rows(torch.arange(2 * 3 * 2 * 1 * 2, dtype=torch.float64).reshape(2, 3, 2, 1, 2), 4)
    assert rows.shape == (3, 4 * 4) and rows[1, 0] == 4 + 2 + 1 and rows[1, 1] == 12 + 4 + 2 + 1 and rows[1, 2] == 0     # first packed tap = tap (1, 0, 1): ci 1 of co 0 | co 1, then the pad lanes


def test_lerp_adjoint_equals_autograd_through_the_oracle():
    """the adjoint of the v1.1 first-chunk interpolation (head of n frames and tail interpolated on their own, modules.py::_interp_v11) as
    vt_time_lerp2x_backward computes it -- weights of the output frames that read a source frame -- against autograd through
    oracle.vidtok_oracle.time_upsample (alpha = 1, zero convolution: the up-sampler IS its interpolation).  The leaf and the cotangent are
    fp64; the oracle's own `_interp_t` casts to fp32 inside, so its gradient carries fp32 rounding of sums of at most four terms with the
    exact weights 1/4, 3/4, 1: the two sides may differ by a few fp32 ulps, 1e-6 relative, and no more"""
    import oracle.vidtok_oracle as O

    def lerp_adjoint(dy):               # dy [B, C, 2 Ti, H, W] -> [B, C, Ti, H, W]
        Ti = dy.shape[2] // 2
        dx = torch.zeros(dy.shape[:2] + (Ti,) + dy.shape[3:], dtype=dy.dtype)
        for j in range(2 * Ti):
            src = max((j + 0.5) * 0.5 - 0.5, 0.0)
            t0 = int(src)
            t1 = t0 + (1 if t0 < Ti - 1 else 0)
            l1 = src - t0
            dx[:, :, t0] += (1 - l1) * dy[:, :, j]
            dx[:, :, t1] += l1 * dy[:, :, j]
        return dx

    Cc = 2
    sd = {"u.mix_factor": torch.tensor([50.0]), "u.conv.conv.weight": torch.zeros((Cc, Cc, 3, 3, 3)), "u.conv.conv.bias": torch.zeros((Cc,))}
    assert torch.sigmoid(sd["u.mix_factor"]).item() == 1.0
    gen = torch.Generator().manual_seed(0)
    for T, n in ((1, 1), (3, 1), (5, 2), (2, 2), (6, 2)):
        x = torch.randn((1, Cc, T, 3, 4), generator=gen, dtype=torch.float64, requires_grad=True)
        up = O.time_upsample(sd, "u", x, "v1_1", O.ChunkState(), "trilinear", n)
        assert up.shape[2] == 2 * T
        dy = torch.randn(up.shape, generator=gen, dtype=torch.float64)
        (up * dy).sum().backward()
        hn = min(n, T)
        got = torch.zeros_like(x)
        got[:, :, :hn] = lerp_adjoint(dy[:, :, :2 * hn])
        if T > n:
            got[:, :, n:] = lerp_adjoint(dy[:, :, 2 * hn:])
        assert ((got - x.grad).abs().max() / x.grad.abs().max()).item() <= 1e-6, (T, n)
