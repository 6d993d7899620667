"""PatchGAN discriminator, everything that needs no GPU: the restatement against the reference class and against the recorded golden,
the parity-class table of the data gradient and the domain of vt_conv_dgrad, refusals, state_dict / checkpoint loading, repacking, the C-ABI surface."""
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

import patchgan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", R.GOLDEN)
# the golden is the same fp64 torch statements run on another machine: equal up to the summation order of its CPU kernels -- n eps with
# n ~ 1e4 terms a sum, through five layers and three normalisations; 1e-9 is far above that and far below any real difference
TOL = 1e-9
NEW_SYMBOLS = ("vt_batchnorm_stats_work_bytes", "vt_batchnorm_stats", "vt_batchnorm_act", "vt_batchnorm_act_backward_work_bytes",
               "vt_batchnorm_act_backward", "vt_leaky_relu_backward")


def _cases():
    return [(si, shape, train) for si, shape in enumerate(R.SHAPES) for train in (True, False)]


# ---- (a) the restatement against the unmodified reference class ------------------------------------------------------------------
@pytest.mark.reference
def test_restatement_equals_reference():
    from oracle import refload

    refload._install_stubs()
    from vidtok.modules.discriminator import NLayerDiscriminator as RefD

    torch.set_num_threads(8)
    ours, ref = R.seeded(), R.seeded(cls=RefD)
    sa, sb = ours.state_dict(), ref.state_dict()
    assert list(sa) == list(sb) and all(sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k]) for k in sa)
    for si, shape, train in _cases():
        x = R.make_inputs(shape, si)
        a, b = R.run64(ours, x, train, seed=si), R.run64(ref, x, train, seed=si)
        assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["dx"], b["dx"]), (shape, train)
        assert all(torch.equal(a["grads"][k], b["grads"][k]) for k in b["grads"]) and set(a["grads"]) == set(b["grads"])
        assert all(torch.equal(a["stats"][k], b["stats"][k]) for k in b["stats"])


# ---- (b) the restatement against the golden recorded from the reference ------------------------------------------------------------------
def test_restatement_equals_golden():
    from safetensors import safe_open

    torch.set_num_threads(8)
    net = R.seeded()
    with safe_open(GOLDEN, "pt") as f:
        keys = json.loads(f.metadata()["keys"])
        gold = {k: f.get_tensor(k) for k in f.keys()}
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == keys and list(net.state_dict()) == list(keys)
    for si, shape, train in _cases():
        r = R.run64(net, R.make_inputs(shape, si), train, seed=si)
        tag = f"s{si}.{'train' if train else 'eval'}."
        for name, got in (("logits", r["logits"]), ("dx", r["dx"])):
            assert got.shape == gold[tag + name].shape and R.rel_max(got, gold[tag + name]) <= TOL, (tag, name)
        for k, g in r["grads"].items():
            assert abs(float(g.norm()) - float(gold[tag + "gnorm." + k])) <= TOL * float(gold[tag + "gnorm." + k]), (tag, k)
            head = gold[tag + "ghead." + k]
            assert (g.reshape(-1)[:64] - head).abs().max() <= TOL * max(float(g.abs().max()), 1e-300), (tag, k)
        for k, v in r["stats"].items():
            assert R.rel_max(v, gold[tag + "stat." + k]) <= TOL or torch.equal(v, gold[tag + "stat." + k]), (tag, k)


# ---- (c) the parity classes of the strided data gradient ---------------------------------------------------------------------------------
GEOMS = [  # (kh, kw, sh, sw, ph, pw, ph_hi, pw_hi, H, W)
    (4, 4, 2, 2, 1, 1, 1, 1, 9, 12),
    (4, 4, 2, 2, 1, 1, 1, 1, 8, 7),
    (3, 3, 2, 2, 0, 0, 1, 1, 9, 8),
    (4, 4, 1, 1, 1, 1, 1, 1, 5, 4),
]


@pytest.mark.parametrize("geom", GEOMS)
def test_strided_dgrad_classes(geom):
    from vidtok_amd.packing import strided_dgrad_classes

    kh, kw, sh, sw, ph, pw, ph_hi, pw_hi, H, W = geom
    classes = strided_dgrad_classes(kh, kw, sh, sw, ph, pw, H, W)
    assert len(classes) == sh * sw
    taps = sorted((p, q) for ch, cw in classes for p in ch["taps"] for q in cw["taps"])
    assert taps == [(p, q) for p in range(kh) for q in range(kw)]            # every tap in exactly one class: they add up to KH * KW
    assert sum(ch["n"] * cw["n"] for ch, cw in classes) == H * W
    # integer-valued fp64 operands: every sum is exact, so the class convolutions must reproduce autograd with error 0
    g = torch.Generator().manual_seed(3)
    cin, cout, B = 3, 5, 2
    w = torch.randint(-3, 4, (cout, cin, kh, kw), generator=g).double()
    x = torch.zeros(B, cin, H, W, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.pad(x, (pw, pw_hi, ph, ph_hi)), w, stride=(sh, sw))
    dy = torch.randint(-4, 5, y.shape, generator=g).double()
    (y * dy).sum().backward()
    dx = torch.zeros(B, cin, H, W, dtype=torch.float64)
    for ch, cw in classes:
        assert ch["pad"] >= 0 and cw["pad"] >= 0
        if not ch["taps"] or not cw["taps"] or ch["n"] == 0 or cw["n"] == 0:
            continue
        sub = w[:, :, ch["taps"]][:, :, :, cw["taps"]].transpose(0, 1)        # flipped taps, Cin / Cout transposed: [cin, cout, nkh, nkw]
        nkh, nkw = len(ch["taps"]), len(cw["taps"])
        # stride-1 convolution of dy under the class's front pads; rows / columns past dy's end read zeros
        need_h, need_w = ch["n"] + nkh - 1, cw["n"] + nkw - 1
        dyp = F.pad(dy, (cw["pad"], max(0, need_w - cw["pad"] - dy.shape[3]), ch["pad"], max(0, need_h - ch["pad"] - dy.shape[2])))
        out = F.conv2d(dyp, sub)[:, :, :ch["n"], :cw["n"]]
        dx[:, :, ch["r"]::sh, cw["r"]::sw] = out
    assert torch.equal(dx, x.grad), float((dx - x.grad).abs().max())


@pytest.mark.parametrize("k", [(3, 3, 1, 1), (4, 4, 1, 1), (1, 3, 0, 1)], ids=["k3 p1", "k4 p1", "1x3 p01"])
def test_stride_one_is_one_class_with_mirrored_pads(k):
    """at stride 1 the class table is the table dgrad_by_forward_conv (tests/test_decoder_backward_host.py) assumes: one class, every tap
    flipped, front pad K - 1 - p, every pixel"""
    from vidtok_amd.packing import strided_dgrad_classes

    kh, kw, ph, pw = k
    H, W = 5, 7
    classes = strided_dgrad_classes(kh, kw, 1, 1, ph, pw, H, W)
    assert len(classes) == 1
    ch, cw = classes[0]
    assert ch["taps"] == list(range(kh))[::-1] and cw["taps"] == list(range(kw))[::-1]
    assert (ch["pad"], cw["pad"]) == (kh - 1 - ph, kw - 1 - pw) and (ch["n"], cw["n"]) == (H, W) and (ch["r"], cw["r"]) == (0, 0)


# ---- (d) refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    from vidtok_amd import lib as L
    from vidtok_amd.discriminator import NLayerDiscriminator

    with pytest.raises(NotImplementedError):
        NLayerDiscriminator(use_actnorm=True)
    with pytest.raises(ValueError):
        NLayerDiscriminator(ndf=12)
    d = NLayerDiscriminator(ndf=8)
    with pytest.raises(NotImplementedError, match="fp16 has no loss scaling"):
        d.set_compute_dtype(torch.float16)
    x = torch.zeros(2, 3, 16, 16)
    for fn in (d.forward, d.forward_with_grad):
        with pytest.raises(L.VtError, match="GPU only"):
            fn(x)
        with pytest.raises(NotImplementedError, match="NCHW"):
            fn(torch.zeros(1, 3, 2, 16, 16))
        with torch.autocast("cpu", dtype=torch.float16):
            with pytest.raises(NotImplementedError, match="fp16 has no loss scaling"):
                fn(x)


# ---- (e) loading and repacking -------------------------------------------------------------------------------------------------------------
def test_state_dict_checkpoint_and_repack(tmp_path):
    from vidtok_amd.discriminator import NLayerDiscriminator, weights_init

    ref = R.seeded(ndf=16)
    d = NLayerDiscriminator(ndf=16)
    assert list(d.state_dict()) == list(ref.state_dict())
    d.load_state_dict(ref.state_dict(), strict=True)
    assert all(torch.equal(v, ref.state_dict()[k]) for k, v in d.state_dict().items())
    ck = {"state_dict": {"loss.discriminator." + k: v for k, v in ref.state_dict().items()}}
    ck["state_dict"].update({"encoder.conv_in.weight": torch.zeros(3), "loss.perceptual_loss.lin0.model.1.weight": torch.zeros(2)})
    path = str(tmp_path / "ckpt.pt")
    torch.save(ck, path)
    d2 = NLayerDiscriminator.from_checkpoint(path, ndf=16)
    assert all(torch.equal(v, ref.state_dict()[k]) for k, v in d2.state_dict().items())
    with pytest.raises(KeyError):
        NLayerDiscriminator.from_checkpoint(path, prefix="loss.nothing.", ndf=16)
    # the packed rows follow the parameter's version counter: an in-place update (optimizer.step) repacks, a second ask does not
    w0, b0 = d._forward_pack(0, torch.float32)
    assert tuple(w0.shape) == (16, 16 * 8) and d._forward_pack(0, torch.float32)[0] is w0
    with torch.no_grad():
        d.main[0].weight.add_(1.0)
    w1, _ = d._forward_pack(0, torch.float32)
    assert w1 is not w0 and torch.equal(w1.reshape(16, 16, 8)[:, :, :3], (w0.reshape(16, 16, 8)[:, :, :3] + 1.0))
    assert bool((w1.reshape(16, 16, 8)[:, :, 3:] == 0).all())
    # weights_init: the reference's hook under the same name
    torch.manual_seed(0)
    d.apply(weights_init)
    assert abs(float(d.main[2].weight.detach().std()) - 0.02) < 2e-3 and abs(float(d.main[3].weight.detach().mean()) - 1.0) < 2e-2 and bool((d.main[3].bias == 0).all())


# ---- (f) the C-ABI surface -------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_and_bound(built_lib):
    from vidtok_amd import lib as L

    with open(os.path.join(ROOT, "include", "vidtok_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in L.SIGNATURES and getattr(built_lib, name) is not None


def test_conv_dgrad_domain(built_lib):
    """vt_conv_dgrad serves st = 1 with sh, sw in {1, 2}; a stride takes a zero time pad, no ups, at most 4 taps an axis and class pads
    that are not negative.  Host side: vt_conv_dgrad_work_bytes is the byte count, or -1 with a message"""
    import ctypes as C

    from vidtok_amd import lib as L
    from vidtok_amd.packing import strided_axis_class

    def desc(**kw):
        d = L.DgradDesc()
        d.B, d.Ti, d.Hi, d.Wi, d.lddx, d.Cin = 2, 1, 9, 12, 16, 12
        d.To, d.Ho, d.Wo, d.lddy, d.Cout = 1, 4, 6, 24, 20
        d.KT, d.KH, d.KW, d.st, d.sh, d.sw = 1, 4, 4, 1, 2, 2
        d.ph = d.pw = d.ph_hi = d.pw_hi = 1
        d.dtype = d.dx_dtype = L.VT_F32
        d.ldw = 4 * 24
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def refused(d, word):
        assert built_lib.vt_conv_dgrad_work_bytes(C.byref(d)) == -1
        msg = built_lib.vt_last_error().decode()
        assert msg.startswith("vt_conv_dgrad:") and word in msg, msg

    # four classes of 5 x 6, 5 x 6, 4 x 6, 4 x 6 pixels, fp32 rows of lddx, each rounded up to 256 bytes
    want = sum((2 * nh * nw * 16 * 4 + 255) // 256 * 256 for nh in (5, 4) for nw in (6, 6))
    assert built_lib.vt_conv_dgrad_work_bytes(C.byref(desc())) == want
    refused(desc(Ho=5), "extents")                                        # not the forward's extent
    refused(desc(st=2, To=1), "strides")
    refused(desc(sh=3, Ho=3), "strides")
    refused(desc(ups_s=1, Ho=9, Wo=12), "no folded up-sampling")          # the extents of the up-sampled 18 x 24 input
    refused(desc(tmode=L.VT_TPAD_REPLICATE), "zero time pad")
    refused(desc(tmode=L.VT_TPAD_CACHE), "tmode")
    refused(desc(KH=5, ph=2, Ho=5, ldw=6 * 24), "1 .. 4 taps")            # (9 + 2 + 1 - 5) / 2 + 1 rows; three row taps a class at the most
    refused(desc(ph=4), "smaller than its kernel extent")
    # a negative class pad: KH = 2, sh = 2, ph = 1: row class 1 holds the one tap 0, and (r + p) / s = 1 > nk - 1 = 0
    ch = strided_axis_class(2, 2, 1, 1, 9)
    assert ch["pad"] == len(ch["taps"]) - 1 - (1 + 1) // 2 == -1
    refused(desc(KH=2, ph=1, ph_hi=0, Ho=5, ldw=2 * 24), "in front of dy's first pixel")      # (9 + 1 + 0 - 2) / 2 + 1 rows
    # K < s: the class no tap reaches has nk = 0, so its pad nk - 1 - (r + p) / s is negative as well: refused like the above
    ch = strided_axis_class(1, 2, 0, 1, 9)
    assert ch["taps"] == [] and ch["pad"] == -1
    refused(desc(KH=1, ph=0, ph_hi=0, Ho=5, ldw=2 * 24), "in front of dy's first pixel")      # (9 - 1) / 2 + 1 rows
    # a class without a pixel (extent <= r) takes no launch and no workspace: one row, so row class 1 is empty
    d = desc(Hi=1, Ho=1, KH=2, ph=0, ph_hi=1, ldw=2 * 24)                                     # (1 + 0 + 1 - 2) / 2 + 1 = 1 row; taps {0}, {1}: pads 0, 0
    assert built_lib.vt_conv_dgrad_work_bytes(C.byref(d)) == 2 * ((2 * 1 * 6 * 16 * 4 + 255) // 256 * 256)
    # stride 1 on the same entry: plain fp32 geometries need no workspace, everything else one exact, unpadded fp32 copy
    d = desc(sh=1, sw=1, Ho=8, Wo=11, ldw=16 * 24)
    assert built_lib.vt_conv_dgrad_work_bytes(C.byref(d)) == 0
    d.tmode, d.KT, d.pt, d.ldw = L.VT_TPAD_REPLICATE, 2, 1, 2 * 16 * 24
    assert built_lib.vt_conv_dgrad_work_bytes(C.byref(d)) == 2 * (1 + 1) * 9 * 12 * 16 * 4
