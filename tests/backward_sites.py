"""Backward operands of every decoder site, for the tests of vt_conv_wgrad / vt_layernorm_act_backward (TEST INFRASTRUCTURE).

`decoder_sites(key)` runs `oracle.vidtok_oracle.decoder_forward` once on the CPU in fp32 with `requires_grad` leaves for every
`decoder.*` parameter and with the module's `causal_conv`, `conv2d_frames`, `layernorm_c` and `silu` wrapped for the duration of the
call, back-propagates a seeded cotangent, and returns what each convolution and each LayerNorm site saw and received:

  ConvSite  x_in (the tensor handed to the convolution, NCTHW), dy (gradient of its output), weight.grad, bias.grad
  NormSite  y_pre (the pre-norm rows), silu (is the site followed by SiLU), d_out (gradient of the fused forward op's output:
            behind the SiLU where there is one), dy_pre (gradient reaching y_pre THROUGH the norm only), gamma.grad, beta.grad

`kernel_conv_operands` / `kernel_norm_operands` turn a site into what the engine would hand the kernel: the geometry and time-pad
mode come from the engine's own conv-site objects (`packing.ConvSite`: `.geom`, `.clip_tmode`), activations go
NCTHW -> NDHWC with `ops.pad_channels` stored channels whose pad lanes carry garbage.  The per-site fp64 references (`ref_wgrad`,
`ref_wgrad_taps`, `ref_ln`) are computed from exactly those operands.
"""
import dataclasses
import functools
from typing import Optional

import torch
import torch.nn.functional as F

from util import build_model, build_oracle

MODELS = {"v1_0": "vidtok_kl_causal_488_4chn", "v1_1": "vidtok_v1_1/vidtok_kl_causal_488_4chn_v1_1"}
LATENT = (1, 4, 3, 5, 6)          # 4x8x8 models: 40 x 48 frames at the widest level -- H != W, no extent a multiple of 32


# ---- fp64 references ------------------------------------------------------------------------------------------------------
def virtual_input(x, g, tmode):
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


def ref_wgrad(x, dy, g, cin, cout, tmode, ref_dtype=torch.float64):
    """(dW, db) by torch autograd on the CPU (fp64 unless asked otherwise), from the same (rounded) operands the kernel reads"""
    xv = virtual_input(x.cpu().to(ref_dtype), g, tmode)[:, :cin]
    w = torch.zeros((cout, cin, g.kt, g.kh, g.kw), dtype=ref_dtype, requires_grad=True)
    b = torch.zeros((cout,), dtype=ref_dtype, requires_grad=True)
    y = F.conv3d(xv, w, b, stride=(g.st, g.sh, g.sw))
    dyc = dy.cpu().to(ref_dtype)[..., :cout].permute(0, 4, 1, 2, 3)
    assert y.shape == dyc.shape, (y.shape, dyc.shape)
    (y * dyc).sum().backward()
    return w.grad, b.grad


def ref_wgrad_taps(x, dy, g, cin, cout, tmode, ref_dtype=torch.float64):
    """the same (dW, db) written out tap by tap: dW[:, :, a, p, q] = sum over output pixels of dy (x) the strided window of the virtual
    input that tap (a, p, q) reads -- one fp64 GEMM per tap, which the large sites need (torch's fp64 conv3d backward is a scalar
    loop); `test_backward_host.py` holds it to `ref_wgrad`"""
    xv = virtual_input(x.cpu().to(ref_dtype), g, tmode)[:, :cin]
    dyc = dy.cpu().to(ref_dtype)[..., :cout].permute(0, 4, 1, 2, 3)
    _B, _C, To, Ho, Wo = dyc.shape
    assert (To, Ho, Wo) == tuple((n - k) // s + 1 for n, k, s in zip(xv.shape[2:], (g.kt, g.kh, g.kw), (g.st, g.sh, g.sw))), (xv.shape, dyc.shape)
    dyf = dyc.permute(1, 0, 2, 3, 4).reshape(cout, -1)
    dw = torch.empty((cout, cin, g.kt, g.kh, g.kw), dtype=ref_dtype)
    for a in range(g.kt):
        for p in range(g.kh):
            for q in range(g.kw):
                win = xv[:, :, a:a + (To - 1) * g.st + 1:g.st, p:p + (Ho - 1) * g.sh + 1:g.sh, q:q + (Wo - 1) * g.sw + 1:g.sw]
                dw[:, :, a, p, q] = dyf @ win.permute(1, 0, 2, 3, 4).reshape(cin, -1).t()
    return dw, dyf.sum(dim=1)


def ref_ln(y, dn, gamma, beta, c, silu, eps, ref_dtype=torch.float64):
    """(dx, dgamma, dbeta) of LayerNorm(+SiLU) over the first c channels of channels-last rows, by torch autograd on the CPU"""
    yv = y.to(ref_dtype).cpu()[..., :c].clone().requires_grad_(True)
    gm = gamma.to(ref_dtype).cpu().clone().requires_grad_(True)
    bt = beta.to(ref_dtype).cpu().clone().requires_grad_(True)
    n = F.layer_norm(yv, (c,), gm, bt, eps)
    if silu:
        n = F.silu(n)
    (n * dn.to(ref_dtype).cpu()[..., :c]).sum().backward()
    return yv.grad, gm.grad, bt.grad


# ---- the recording pass ---------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class ConvSite:
    name: str                       # state-dict prefix: <name>.weight, <name>.bias
    x_in: torch.Tensor              # NCTHW, what the oracle handed the convolution (before its padding)
    dy: torch.Tensor                # NCTHW, gradient of the convolution's output
    dw: torch.Tensor                # whole-graph weight.grad (reference layout of the state dict: rank 3, 4 or 5)
    db: Optional[torch.Tensor]


@dataclasses.dataclass
class NormSite:
    name: str                       # state-dict prefix: <name>.weight (gamma), <name>.bias (beta)
    y_pre: torch.Tensor             # NCTHW pre-norm rows
    silu: bool
    d_out: torch.Tensor             # NCTHW, dn of ops.layernorm_act_backward
    dy_pre: torch.Tensor            # NCTHW, gradient of y_pre through this norm only
    dgamma: torch.Tensor
    dbeta: torch.Tensor


@functools.lru_cache(maxsize=1)
def decoder_sites(key, seed=11):
    """(engine model, conv sites, norm sites, leaves) of one whole-decoder fp32 autograd pass on the CPU; `leaves` maps every
    `decoder.*` key of the state dict to its requires_grad tensor (grad filled in)"""
    import oracle.vidtok_oracle as O

    model, cfg, sd = build_model(MODELS[key], seed=seed)
    eng = build_oracle(cfg, sd)
    assert eng.version == key
    leaves = {k: v.detach().float().clone().requires_grad_(True) for k, v in sd.items() if k.startswith("decoder.")}
    name_of = {id(v): k for k, v in leaves.items()}
    convs, norms, by_out, keep = [], [], {}, []
    orig = {n: getattr(O, n) for n in ("causal_conv", "conv2d_frames", "layernorm_c", "silu")}

    def rec_conv(fn):
        def wrapped(sd_, name, x, *a, **kw):
            y = fn(sd_, name, x, *a, **kw)
            y.retain_grad()
            convs.append((name, x, y))
            return y
        return wrapped

    def rec_norm(x, w, b, eps=1e-6):
        assert eps == 1e-6
        xin = x.clone()                 # a node of its own: its gradient is the norm's alone, not the residual path's as well
        xin.retain_grad()
        n = orig["layernorm_c"](xin, w, b, eps)
        n.retain_grad()
        gname = name_of[id(w)]
        assert gname.endswith(".weight") and name_of[id(b)] == gname[:-len("weight")] + "bias"
        site = dict(name=gname[:-len(".weight")], y=xin, n=n, act=None)
        norms.append(site)
        by_out[id(n)] = site
        keep.append(n)                  # ids stay unique while the tensors live
        return n

    def rec_silu(x):
        out = orig["silu"](x)
        site = by_out.get(id(x))
        if site is not None:
            assert site["act"] is None
            out.retain_grad()
            site["act"] = out
        return out

    O.causal_conv, O.conv2d_frames, O.layernorm_c, O.silu = rec_conv(orig["causal_conv"]), rec_conv(orig["conv2d_frames"]), rec_norm, rec_silu
    try:
        z = torch.randn(LATENT, generator=torch.Generator().manual_seed(seed + 1))
        out = O.decoder_forward(leaves, eng.dec_params, z, eng.version, O.ChunkState())
    finally:
        for n, f in orig.items():
            setattr(O, n, f)
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed + 2))
    (out * cot).sum().backward()

    conv_sites = [ConvSite(name, x.detach(), y.grad, leaves[name + ".weight"].grad,
                           leaves[name + ".bias"].grad if (name + ".bias") in leaves else None) for name, x, y in convs]
    norm_sites = []
    for s in norms:
        silu = s["act"] is not None
        # the call sites decide: resnet blocks and norm_out feed a SiLU, the attention norm does not
        assert silu == (not s["name"].endswith(".attn_1.norm.norm")), s["name"]
        norm_sites.append(NormSite(s["name"], s["y"].detach(), silu, (s["act"] if silu else s["n"]).grad, s["y"].grad,
                                   leaves[s["name"] + ".weight"].grad, leaves[s["name"] + ".bias"].grad))
    return model, conv_sites, norm_sites, leaves


def expected_parameters(leaves):
    """every decoder.* parameter a site has to account for: all of them but the up-samplers' scalar mix factors"""
    return {k for k in leaves if not k.endswith(".mix_factor")}


def compared_parameters(conv_sites, norm_sites):
    """parameter names the site table covers; a parameter fed by two sites would need its gradients added, and none is"""
    names = [s.name for s in conv_sites] + [s.name for s in norm_sites]
    assert len(names) == len(set(names)), "a parameter receives gradient from more than one site"
    out = set()
    for s in conv_sites:
        out |= {s.name + ".weight"} | ({s.name + ".bias"} if s.db is not None else set())
    for s in norm_sites:
        out |= {s.name + ".weight", s.name + ".bias"}
    return out


# ---- site -> kernel operands ----------------------------------------------------------------------------------------------
def site_geometry(model, site: ConvSite):
    """(ConvGeom, tmode, pre-up-sample NCTHW input) the engine's own site object gives for this convolution on a whole clip"""
    from vidtok_amd import modules as M

    owner = model.get_submodule(site.name.rsplit(".", 1)[0])
    x = site.x_in
    if isinstance(owner, M.Upsample):             # nearest x2 in space, folded into the gather of the training path's one launch
        s = owner.fold_site
        assert s.geom.ups_s == 1 and torch.equal(x[..., 0::2, 0::2], x[..., 1::2, 1::2])       # the folded up-sampling really is a repetition
        return s.geom, s.clip_tmode, x[..., 0::2, 0::2]
    if hasattr(owner, "_tmode_and_cache"):        # a causal convolution: the owner holds the chunk state
        s = owner.site
        tmode, cache = owner._tmode_and_cache(owner.version, owner.time_pad)
        assert cache is None and tmode == s.clip_tmode                                           # a whole clip: no chunk-to-chunk cache form
        up = model.get_submodule(site.name.rsplit(".", 2)[0])
        if isinstance(up, M.TimeUpsampleResCausal2x) and not (up.version == "v1_1" and up.enable_cached):
            # nearest x2 in time, folded into the gather: the kernel reads the tensor in front of the up-sampling
            assert torch.equal(x[:, :, 0::2], x[:, :, 1::2])
            return dataclasses.replace(s.geom, ups_t=1), tmode, x[:, :, 0::2]
        return s.geom, tmode, x                   # (v1.1 trilinear: the interpolated tensor as it was convolved)
    s = next(s for s in owner.sites if s is not None and s.conv is model.get_submodule(site.name))
    return s.geom, s.clip_tmode, x


def to_ndhwc(t, ld, dtype, seed):
    """NCTHW -> NDHWC with ld stored channels; the pad lanes carry garbage no result may depend on"""
    B, C, T, H, W = t.shape
    out = 1.0 + 3.0 * torch.randn((B, T, H, W, ld), generator=torch.Generator().manual_seed(seed))
    out[..., :C] = t.permute(0, 2, 3, 4, 1)
    return out.to(dtype)


def kernel_conv_operands(model, site: ConvSite, dtype):
    """(x NDHWC, dy NDHWC, geom, cin, cout, tmode) for ops.conv_wgrad, operands rounded to `dtype`"""
    from vidtok_amd import ops

    g, tmode, x = site_geometry(model, site)
    cin, cout = x.shape[1], site.dy.shape[1]
    return to_ndhwc(x, ops.pad_channels(cin), dtype, 1), to_ndhwc(site.dy, ops.pad_channels(cout), dtype, 2), g, cin, cout, tmode


def kernel_norm_operands(site: NormSite, leaves, dtype):
    """(y rows, dn rows, gamma, beta, c) for ops.layernorm_act_backward, rows rounded to `dtype`"""
    from vidtok_amd import ops

    c = site.y_pre.shape[1]
    ld = ops.pad_channels(c)
    return (to_ndhwc(site.y_pre, ld, dtype, 3), to_ndhwc(site.d_out, ld, dtype, 4), leaves[site.name + ".weight"].detach(),
            leaves[site.name + ".bias"].detach(), c)


def weight5(dw):
    """a state-dict weight gradient (Conv1d over time, Conv2d per frame, Conv3d) in the kernel's [cout, cin, kt, kh, kw] layout"""
    return dw[:, :, :, None, None] if dw.dim() == 3 else (dw[:, :, None] if dw.dim() == 4 else dw)


# ---- geometries of the unit grid the decoder does not have (tests/test_gpu_backward_ops.py, part B) ------------------------------
def edge_geoms():
    """name -> (ConvGeom, time-pad modes): the strided forms of the encoder, the centred time pad of the non-causal family, the
    2x2 phase kernels of `Upsample`, folded up-sampling under a replicate pad"""
    from vidtok_amd import lib as L
    from vidtok_amd.ops import ConvGeom

    Z, R = L.VT_TPAD_ZERO, L.VT_TPAD_REPLICATE
    out = {
        "downsample 3x3 s2": (ConvGeom(kh=3, kw=3, sh=2, sw=2, ph=0, pw=0, ph_hi=1, pw_hi=1), (Z,)),
        "time-down 3x3x3 st2": (ConvGeom(kt=3, kh=3, kw=3, st=2, pt=1, ph=1, pw=1, ph_hi=1, pw_hi=1), (Z, R)),
        "time-down 3x1x1 st2": (ConvGeom(kt=3, st=2, pt=1), (Z, R)),
        "1x3x3 s21": (ConvGeom(kh=3, kw=3, sh=2, sw=1, ph=0, pw=1, ph_hi=1, pw_hi=1), (Z,)),          # row and column strides differ
        "3x3x3 s222": (ConvGeom(kt=3, kh=3, kw=3, st=2, sh=2, sw=2, pt=1, ph=0, pw=0, ph_hi=1, pw_hi=1), (Z, R)),
        "centred 3x3x3": (ConvGeom(kt=3, kh=3, kw=3, pt=1, pt_hi=1, ph=1, pw=1, ph_hi=1, pw_hi=1), (Z,)),
        "centred 3x1x1": (ConvGeom(kt=3, pt=1, pt_hi=1), (Z,)),
        "up_t 3x3x3": (ConvGeom(kt=3, kh=3, kw=3, pt=2, ph=1, pw=1, ph_hi=1, pw_hi=1, ups_t=1), (Z, R)),
        "up_s 1x3x3": (ConvGeom(kh=3, kw=3, ph=1, pw=1, ph_hi=1, pw_hi=1, ups_s=1), (Z,)),
        "up_t up_s 3x3x3": (ConvGeom(kt=3, kh=3, kw=3, pt=2, ph=1, pw=1, ph_hi=1, pw_hi=1, ups_t=1, ups_s=1), (Z, R)),
        "1x3x3": (ConvGeom(kh=3, kw=3, ph=1, pw=1, ph_hi=1, pw_hi=1), (Z,)),
        "1x1x1": (ConvGeom(), (Z,)),
    }
    for py in (0, 1):
        for px in (0, 1):
            out[f"phase 2x2 {py}{px}"] = (ConvGeom(kh=2, kw=2, ph=1 - py, pw=1 - px, ph_hi=py, pw_hi=px), (Z,))
    return out


def wgrad_plan(M, K, cout):
    """(ranges, pixels per range, workspace bytes) of vt_conv_wgrad by its documented rule (csrc/grad.hip, vidtok_amd.h): 64 x 64
    tiles of dW, 32-pixel stages; enough ranges to fill the chip twice over (2048 workgroups), each at least 8 stages long, 64 at the
    most; the stages dealt out evenly and the range count recomputed from that; one fp32 partial [cout][K] and one [cout] per range,
    each block rounded up to 256 bytes"""
    cdiv = lambda a, b: (a + b - 1) // b  # noqa: E731
    tiles, stages = cdiv(K, 64) * cdiv(cout, 64), cdiv(M, 32)
    ns = max(1, min(cdiv(2048, tiles), stages // 8, 64))
    per = cdiv(stages, ns)
    ns = cdiv(stages, per)
    return ns, per * 32, cdiv(ns * cout * K * 4, 256) * 256 + cdiv(ns * cout * 4, 256) * 256


def ln_backward_plan(M, C):
    """(workgroups, rows per workgroup, workgroups that own no row, workspace bytes) of vt_layernorm_act_backward: 32 rows per
    workgroup, 4096 workgroups at the most, the rows dealt out evenly; two fp32 partial blocks [workgroups][C]"""
    cdiv = lambda a, b: (a + b - 1) // b  # noqa: E731
    groups = max(1, min(cdiv(M, 32), 4096))
    rows = cdiv(M, groups)
    return groups, rows, groups - cdiv(M, rows), 2 * cdiv(groups * C * 4, 256) * 256
