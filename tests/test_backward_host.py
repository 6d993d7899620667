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
