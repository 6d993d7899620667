"""LPIPS without a GPU: the restatement (tests/lpips_ref.py) against the unmodified reference and its golden values, the module's keys,
the weight-file handling, and the argument checks of the new C entry points (which return before any device work)."""
import ctypes as C
import os
import socket

import pytest
import torch
from safetensors.torch import load_file

import lpips_ref
from lpips_cases import CASES, lpips_state_dict, make_inputs
from util import GOLDEN_DIR


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def _shapes():
    from vidtok_amd.lpips import LPIPS

    return {k: v.shape for k, v in LPIPS(pretrained=False).state_dict().items()}


def _restated(case, sd):
    x, y = make_inputs(case)
    with torch.no_grad():
        if case["form"] == "eval":
            v, taps = lpips_ref.eval_frames(sd, x, y, with_taps=True)
            return v.reshape(-1), taps
        return lpips_ref.lpips(sd, x, y, with_taps=True)


@pytest.mark.reference
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_equals_reference(case):
    from lpips_refload import reference_lpips

    ref = reference_lpips(use_dropout=True)
    sd = lpips_state_dict({k: v.shape for k, v in ref.state_dict().items()})
    ref.load_state_dict(sd, strict=True)
    x, y = make_inputs(case)
    with torch.no_grad():
        if case["form"] == "eval":
            want = lpips_ref.eval_frames(sd, x, y).reshape(-1)
            o = y.clamp(-1, 1)
            inp, o = (x + 1) / 2, (o + 1) / 2
            B, Cc, T, H, W = x.shape
            inp = inp.permute(0, 2, 1, 3, 4).reshape(B * T, Cc, H, W)
            o = o.permute(0, 2, 1, 3, 4).reshape(B * T, Cc, H, W)
            got = ref(inp * 2 - 1, o * 2 - 1).reshape(-1)
        else:
            want, got = lpips_ref.lpips(sd, x, y), ref(x, y).reshape(-1)
    assert _rel(want, got) <= 1e-6


@pytest.mark.reference
@pytest.mark.parametrize("use_dropout", [True, False])
def test_module_keys_equal_reference(use_dropout):
    from lpips_refload import reference_lpips

    from vidtok_amd.lpips import LPIPS

    ours = {k: tuple(v.shape) for k, v in LPIPS(use_dropout=use_dropout, pretrained=False).state_dict().items()}
    ref = {k: tuple(v.shape) for k, v in reference_lpips(use_dropout=use_dropout).state_dict().items()}
    assert ours == ref
    sd = reference_lpips(use_dropout=use_dropout).state_dict()
    LPIPS(use_dropout=use_dropout, pretrained=False).load_state_dict(sd, strict=True)    # a reference state_dict loads strictly


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_reproduces_golden(case):
    g = load_file(os.path.join(GOLDEN_DIR, "lpips.safetensors"))
    v, taps = _restated(case, lpips_state_dict(_shapes()))
    assert _rel(v, g[case["name"] + "/lpips"]) <= 1e-5
    assert _rel(taps, g[case["name"] + "/taps"]) <= 1e-5


def test_torchvision_keys_load(tmp_path):
    """a torchvision vgg16 state_dict (features.N.*, classifier.* ignored) and an LPIPS lin file load onto net.sliceK.N.* / linK.*"""
    from lpips_refload import vgg16_features

    from vidtok_amd.lpips import LPIPS

    torch.manual_seed(3)
    feats = {"features." + k: v for k, v in vgg16_features().state_dict().items()}
    feats["classifier.0.weight"] = torch.randn(4, 4)
    lin = {f"lin{k}.model.1.weight": torch.rand(1, c, 1, 1) for k, c in enumerate([64, 128, 256, 512, 512])}
    torch.save(feats, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "vgg.pth")
    m = LPIPS(lpips_ckpt=str(tmp_path / "vgg.pth"), vgg_ckpt=str(tmp_path / "vgg16.pth"))
    sd = m.state_dict()
    assert torch.equal(sd["net.slice1.0.weight"], feats["features.0.weight"])
    assert torch.equal(sd["net.slice3.14.bias"], feats["features.14.bias"])
    assert torch.equal(sd["net.slice5.28.weight"], feats["features.28.weight"])
    assert torch.equal(sd["lin4.model.1.weight"], lin["lin4.model.1.weight"])
    n_conv = sum(1 for k in feats if k.startswith("features.") and k.endswith(".weight"))
    assert n_conv == 13 and sum(1 for k in sd if k.startswith("net.") and k.endswith(".weight")) == 13


def test_missing_weight_files_raise_without_network(tmp_path, monkeypatch):
    from vidtok_amd.lpips import LPIPS

    def refuse(*a, **k):
        raise AssertionError("network access attempted")

    monkeypatch.setattr(socket.socket, "connect", refuse)
    monkeypatch.setattr(socket, "create_connection", refuse)
    a, b = str(tmp_path / "nope" / "vgg.pth"), str(tmp_path / "nope" / "vgg16.pth")
    with pytest.raises(FileNotFoundError) as e:
        LPIPS(lpips_ckpt=a, vgg_ckpt=b)
    assert a in str(e.value) and b in str(e.value)
    import vidtok_amd.lpips as mod

    src = open(mod.__file__).read()
    assert "requests" not in src.split('"""', 2)[2] and "torchvision" not in [ln.split()[1] for ln in src.splitlines() if ln.startswith("import ")]


# ---- argument checks of the C entry points (no device work: every call below must fail validation) -------------------------------
_FAKE = C.c_void_p(1 << 20)          # an aligned address that is never dereferenced


def _err(rc, lib, needle):
    assert rc == -1, rc                  # VT_ERR_ARG
    assert needle in lib.vt_last_error().decode(), lib.vt_last_error().decode()


def _desc(**kw):
    from vidtok_amd import lib as L

    d = L.ConvDesc()
    d.x = d.w = d.y = 1 << 20
    d.B, d.Ti, d.Hi, d.Wi, d.Cin, d.To, d.Ho, d.Wo, d.Cout = 2, 1, 16, 16, 64, 1, 16, 16, 64
    d.ldw, d.ldy, d.KT, d.KH, d.KW, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = 576, 64, 1, 3, 3, 1, 1, 1, 0, 1, 1
    d.dtype = d.out_dtype = L.VT_BF16
    d.nbatch = 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("bad, needle", [
    (dict(act=0), "act"),
    (dict(dtype=2, out_dtype=2), "dtype"),
    (dict(dtype=3, out_dtype=0, ldw=576), "same type"),
    (dict(out_dtype=0), "same type"),
    (dict(x=None), "null"),
    (dict(res_mode=1, res=1 << 20, Tr=1, ldr=64), "residual"),
])
def test_conv_act_rejects(built_lib, bad, needle):
    from vidtok_amd import lib as L

    act = bad.pop("act", L.VT_ACT_RELU)
    d = _desc(**bad)
    _err(built_lib.vt_conv_act(C.byref(d), act, None), built_lib, needle)


def test_lpips_entry_points_reject(built_lib):
    from vidtok_amd import lib as L

    lib = built_lib
    wb = lib.vt_lpips_work_bytes(2, 32, 32)
    assert wb > 0 and lib.vt_lpips_work_bytes(2, 15, 32) == 0 and lib.vt_lpips_work_bytes(2, 32, 8) == 0
    P = _FAKE
    prep = lambda **k: lib.vt_lpips_prep(k.get("x", P), k.get("y", P), k.get("out", P), k.get("shift", P), k.get("scale", P),  # noqa: E731
                                         k.get("dtype", L.VT_BF16), 2, 1, k.get("H", 32), k.get("W", 32), k.get("flags", 0), None)
    _err(prep(dtype=L.VT_I32), lib, "dtype")
    _err(prep(dtype=L.VT_BF16X3), lib, "dtype")
    for name in ("x", "y", "out", "shift", "scale"):
        _err(prep(**{name: None}), lib, "null")
    _err(prep(H=15), lib, "H, W >= 16")
    _err(prep(W=12), lib, "H, W >= 16")
    _err(prep(flags=8), lib, "flags")
    tap = lambda **k: lib.vt_lpips_tap(k.get("feat", P), k.get("pooled", P), k.get("lin", P), k.get("work", P), k.get("wb", wb),  # noqa: E731
                                       k.get("dtype", L.VT_BF16), 2, 32, 32, k.get("C", 64), k.get("tap", 0), None)
    _err(tap(dtype=L.VT_I32), lib, "dtype")
    for c in (3, 8, 32, 96, 1024):
        _err(tap(C=c), lib, "C=")
    for name in ("feat", "lin", "work"):
        _err(tap(**{name: None}), lib, "null")
    _err(tap(wb=wb - 4), lib, "workspace")
    _err(tap(tap=5), lib, "tap")
    _err(tap(feat=C.c_void_p((1 << 20) + 4)), lib, "aligned")
    fin = lambda **k: lib.vt_lpips_finish(k.get("work", P), k.get("wb", wb), k.get("out", P), None, 2, k.get("H", 32), k.get("W", 32), None)  # noqa: E731
    _err(fin(work=None), lib, "null")
    _err(fin(out=None), lib, "null")
    _err(fin(wb=wb - 1), lib, "workspace")
    _err(fin(H=8), lib, "H, W >= 16")
