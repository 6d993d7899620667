"""`-m gpu`: every launch reads and writes only inside its operands (tests/arena.py).

Record, relocate, replay, check: a case of the operator tests runs once on plain torch allocations with the launch record on, every
recorded launch is then replayed with ALL its operands carved out of one 0xFF-filled arena -- slots at odd multiples of 16 bytes, moats
of at least 1 MiB between them, scratch at exactly the size the library asked for -- and the bytes are compared: moats and inputs
untouched, pad lanes unchanged or zero, rows of another launch unchanged, the owned result the bits of the plain run, the plan the plan
of the plain launch.  Operators without a launch record are replayed from the log of their C calls the same way.

Not reproducible run to run by design, so compared inside the operator's own gate instead of bit for bit (and required finite):
vt_groupnorm_act (fp64 atomics over the workgroups of an instance).  Everything else here is held to the same bits."""
import collections
import contextlib
import ctypes as C
import math

import pytest
import torch

import arena as A
import test_gpu_ops as T
from util import rel_err, tup3_operands, tup3_run
from vidtok_amd import lib as L
from vidtok_amd import ops
from vidtok_amd.ops import ConvGeom
from vidtok_amd.packing import pack_conv_weight

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32, X3 = torch.bfloat16, torch.float16, torch.float32, T.X3
DT_ID = {BF16: "bf16", F16: "f16", F32: "f32", X3: "x3"}

REACHED = set()                          # (kernel, tile, lds_epilogue, deep_ring, launches > 1) | ("paired",) | ("tblock",) | ("flash",)
COUNTS = collections.Counter()           # relocated launches per family


@contextlib.contextmanager
def recording():
    """every MFMA-kernel launch of the block, also those of helpers that keep a launch record of their own (_check_conv)"""
    rec, orig = [], ops._conv_launch

    def launch(lib, d, what, keep=()):
        orig(lib, d, what, keep)
        if ops.CONV_RECORD is not rec:
            rec.append((d, keep, None))

    ops._conv_launch, ops.CONV_RECORD = launch, rec
    try:
        yield rec
    finally:
        ops._conv_launch, ops.CONV_RECORD = orig, None


def _replay_check(entry, family, pre=None):
    """one recorded launch in an arena of its own -> (plan or None, arena)"""
    d = entry[0]
    plan = ops.conv_plan(d) if isinstance(d, L.ConvDesc) else None
    ar, d2 = A.relocate(entry, plan=plan, pre=pre, vt_ncthw=L.VT_NCTHW)
    ops.replay_convs([(d2, (), None)], conv_kernel_only=False)
    torch.cuda.synchronize()
    ar.check()
    if plan is not None:
        assert ops.conv_plan(d2) == plan, (ops.conv_plan(d2), plan)                      # (f)
        if d.work:
            assert L.load().vt_conv_work_bytes(C.byref(d2)) == d.work_bytes == ar.slots["work"].nbytes
    if isinstance(d, ops.TimeUp3Desc):
        REACHED.add(("paired",))
    elif isinstance(d, L.TBlockDesc):
        REACHED.add(("tblock",))
    elif isinstance(d, tuple):
        REACHED.add(("flash",))
    else:
        REACHED.add((plan["kernel"], plan["tile"], _lds_epilogue(plan, d), plan["deep_ring"], plan["launches"] > 1))
    COUNTS[family] += 1
    return plan, ar


def _lds_epilogue(plan, d):
    """vt_conv_plan reports the LDS epilogue of the 8-wave tile and of conv_in8; for the 128 x 128 tile, whose full tiles take
    conv_epilogue_lds128, vt_conv_launch_form does"""
    if plan["kernel"] != "igemm" or plan["tile"] != (128, 128):
        return plan["lds_epilogue"]
    return bool(ops.conv_launch_form(d)["lds_epi"])


def _conv_case(case, dtype, family, forms=None):
    """the launch of one case of a table of tests/test_gpu_ops.py, plain and relocated -> (plan, arena); forms: a list that receives
    vt_conv_launch_form of the plain launch"""
    _name, _shape, _cin, cout, _kdims, geom, _ex = case
    x, w, _rows, bias, kw, ln = T._conv_operands(case, dtype)
    with recording() as rec:
        if ln is not None:
            ops.conv(x, w, bias, geom, cout=cout, ln=(ln[0], ln[1], 1e-6, True), ln_keep_y=ln[2], **kw)
        else:
            ops.conv(x, w, bias, geom, cout=cout, **kw)
    torch.cuda.synchronize()
    assert len(rec) == 1
    if forms is not None:
        forms.append(ops.conv_launch_form(rec[0][0]))
    return _replay_check(rec[0], family)


def _params(cases, dtypes):
    return [pytest.param(c, dt, id=f"{c[0]}-{DT_ID[dt]}") for c in cases for dt in dtypes]


# ---- implicit GEMM ------------------------------------------------------------------------------------------------------------------
FOUR_ARITHMETICS = [c for c in T.CONV_CASES if c[0] in ("conv2d_3x3_64_192_ragged", "conv2d_ln_fused", "conv_out_128_3_ncthw_trim")]
assert len(FOUR_ARITHMETICS) == 3


@pytest.mark.parametrize("buf", [1, 0], ids=["descriptors", "pointers"])
@pytest.mark.parametrize("case,dtype", _params(T.CONV_CASES, [BF16, F32]) + _params(FOUR_ARITHMETICS, [X3, F16]))
def test_conv_cases(case, dtype, buf, vt_opts):
    vt_opts(conv_buf=buf)
    forms = []
    plan, _ = _conv_case(case, dtype, "igemm tables (CONV_CASES)", forms=forms)
    # descriptors unless switched off -- or in cache mode, where they need the tap walk (Cin a multiple of the K step) and frames of whole tiles
    if plan["kernel"] == "igemm":
        (_b, Tt, H, W), cin, geom = case[1], case[2], case[5]
        _to, Ho, Wo = geom.out_dims(Tt, H, W)
        step = 64 if dtype in T.H16 else 16 if dtype is X3 and plan["tile"] == (256, 256) else 32
        desc = bool(buf) and (case[6].get("tmode") != "cache" or (cin % step == 0 and (Ho * Wo) % plan["tile"][0] == 0))
        assert forms[0]["gather"] == ("desc" if desc else "ptr") and (forms[0]["x_bytes"] > 0) == desc, forms[0]


@pytest.mark.parametrize("case,dtype", _params(T.BIG256, [BF16, F32]))
def test_conv_forced_256_tile(case, dtype, vt_opts):
    vt_opts(conv_tile=256)
    plan, ar = _conv_case(case, dtype, "igemm 256 tile forced (BIG256)")
    assert plan["tile"] == (256, 256)
    (B, Tt, H, W), cout, ex = case[1], case[3], case[6]
    if "ln" in ex and cout == 256 and (B * Tt * H * W) % 256 == 0:
        assert plan["ln_fused"] and plan["launches"] == 1
        if ex["ln"] == "only":                   # "the fused kernel never writes it": all of y is another's
            assert ar.slots["y"].kind == "out" and not bool(ar.slots["y"].owned.any()) and bool((ar.raw("y") == 0xFF).all())


@pytest.mark.parametrize("ring", ["deep", "deep_pointers", "two_slots"])
@pytest.mark.parametrize("case", T.DEEP_CASES, ids=[c[0] for c in T.DEEP_CASES])
def test_conv_128_tile_rings(case, ring, vt_opts):
    vt_opts(conv_tile=128, conv_ws=0, conv_deep=(0 if ring == "two_slots" else 1), conv_buf=(0 if ring == "deep_pointers" else 1))
    plan, _ = _conv_case(case, BF16, "igemm rings (DEEP_CASES)")
    steps = math.prod(case[4]) * case[2] // 64
    assert plan["tile"] == (128, 128) and plan["deep_ring"] == (ring != "two_slots" and steps >= 8), (plan, steps)


@pytest.mark.parametrize("case,dtype", _params(T.LDSEPI_CASES, [BF16, F32]))
def test_conv_without_lds_epilogue(case, dtype, vt_opts):
    vt_opts(conv_ldsepi=0, conv_ws=0)
    plan, _ = _conv_case(case, dtype, "igemm vector epilogue (LDSEPI_CASES)")
    assert plan["tile"] == (128, 128) and not plan["ln_fused"] and not plan["lds_epilogue"]


def _pixels(case):
    (B, Tt, H, W), geom = case[1], case[5]
    To, Ho, Wo = geom.out_dims(Tt, H, W)
    return B * To * Ho * Wo


# the LDS-transposed epilogue of the 8-wave tile takes full 256-pixel tiles without LayerNorm, NCTHW output or a time-shifted residual:
# the smallest Cout % 256 == 0 case of CONV_CASES of that kind
PLAIN256 = min((c for c in T.BIG256 if _pixels(c) % 256 == 0 and not ({"ln", "ncthw"} & set(c[6])) and c[6].get("res") != "mix_up"),
               key=lambda c: _pixels(c) * c[2] * math.prod(c[4]))


@pytest.mark.parametrize("coalesced", [True, False], ids=["lds_epilogue", "vector_epilogue"])
def test_conv_8wave_plain_epilogues(coalesced, vt_opts):
    vt_opts(conv_tile=256, conv_ldsepi=(1 if coalesced else 0), conv_fuse_ln256=(1 if coalesced else 0))
    plan, _ = _conv_case(PLAIN256, BF16, "igemm 8-wave plain epilogues")
    assert plan["tile"] == (256, 256) and plan["lds_epilogue"] == coalesced, plan


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("cout,tile", [(128, 0), (256, 256)], ids=["lds128_epilogue", "lds256_epilogue"])
def test_conv_streaming_stores(cout, tile, dt, vt_opts):
    """the launches of test_conv_streaming_stores_same_bits; its last one runs with the threshold at 1 MiB: nt stores of y and n"""
    with recording() as rec:
        T.test_conv_streaming_stores_same_bits(cout, tile, dt, vt_opts)
    assert len(rec) == 2 and L.get_option("conv_nt_mb") == 1
    plan, ar = _replay_check(rec[-1], "igemm streaming stores")
    assert ar.slots["y"].nbytes >= 1 << 20 and plan["tile"] == ((256, 256) if tile else (128, 128))


# ---- split-K, weight-stationary, narrow, conv_in ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case,dtype", _params(T.SPLITK_CASES, T.H16))
def test_conv_split_k(case, dtype, vt_opts):
    vt_opts(conv_splitk=1)
    plan, ar = _conv_case(case, dtype, "split-K (SPLITK_CASES)")
    assert plan["launches"] == 2 + (1 if "ln" in case[6] else 0) and ar.slots["work"].kind == "scratch"


WS_SMALL = [c for c in T.WS_CASES if c[0] in ("ws_single_tile", "ws_two_tiles_one_wg", "ws_one_tile_column", "ws_one_tile_row", "ws_3x3_tiles_frames",
                                              "ws_no_bias_path")]
assert len(WS_SMALL) == 6


@pytest.mark.parametrize("case,dtype", _params(WS_SMALL, T.H16))
def test_conv_weight_stationary(case, dtype, vt_opts):
    vt_opts(conv_ws=2)
    plan, _ = _conv_case(case, dtype, "conv_ws2 (WS_CASES)")
    assert plan["kernel"] == "ws2" and ("ln" not in case[6] or plan["ln_fused"])


@pytest.mark.parametrize("case,dtype", _params(T.NARROW_CASES, T.H16))
def test_conv_narrow(case, dtype, vt_opts):
    vt_opts(conv_narrow=1)
    plan, _ = _conv_case(case, dtype, "conv_narrow (NARROW_CASES)")
    assert plan["kernel"] == "narrow"


@pytest.mark.parametrize("case,dtype", _params(T.IN8_CASES, T.H16))
def test_conv_in8(case, dtype, vt_opts):
    vt_opts(conv_in8=1)
    plan, _ = _conv_case(case, dtype, "conv_in8 (IN8_CASES)")
    assert plan["kernel"] == "in8"


# ---- interleaved outputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("cout,hw", [(128, (16, 16)), (256, (8, 8)), (512, (5, 7))])
def test_conv_output_frame_interleave(cout, hw, dtype):
    """the two parity launches of test_conv_output_frame_interleave, each on its own: the other parity's frames stay 0xFF"""
    with recording() as rec:
        T.test_conv_output_frame_interleave(cout, hw, dtype)
    assert len(rec) == 2 and [e[0].yt_off for e in rec] == [0, 1]
    for e in rec:
        _, ar = _replay_check(e, "frame interleave")
        assert int(ar.slots["y"].owned.sum()) * 2 == ar.slots["y"].owned.numel()


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("cout,hw", [(128, (8, 16)), (256, (8, 8)), (512, (5, 7))])
def test_conv_output_pixel_interleave(cout, hw, dtype):
    with recording() as rec:
        T.test_conv_output_pixel_interleave(cout, hw, dtype)
    assert len(rec) == 4 and sorted((e[0].ys_oh, e[0].ys_ow) for e in rec) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for e in rec:
        _, ar = _replay_check(e, "pixel interleave")
        assert int(ar.slots["y"].owned.sum()) * 4 == ar.slots["y"].owned.numel()


@pytest.mark.parametrize("dtype", T.H16, ids=T.H16_IDS)
def test_conv_frame_interleave_with_pad_lanes(dtype):
    """out at ld = Cout + 8 on full 128-pixel tiles (the LDS-transposed epilogue stores 16-byte pieces of rows): lanes 128 .. 135 of the
    owned frames stay as they were or become zero, the other frames stay whole"""
    B, Tt, H, W, cin, cout = 2, 3, 16, 16, 128, 128
    x = T._act(B, Tt, H, W, cin, dtype, 1)
    geom = ConvGeom(kt=2, kh=3, kw=3, pt=1, ph=1, pw=1, ph_hi=1, pw_hi=1)
    g = torch.Generator().manual_seed(2)
    w = pack_conv_weight(torch.randn((cout, cin, 2, 3, 3), generator=g) / math.sqrt(cin * 18), dtype, cin_stored=cin).to(DEV)
    bias, res, mf = T._rand((cout,), F32, 3, 0.1), T._act(B, Tt, H, W, cout, dtype, 4), torch.tensor([0.2], device=DEV)
    y = torch.zeros((B, 2 * Tt, H, W, cout + 8), dtype=dtype, device=DEV)
    with recording() as rec:
        for par in (0, 1):
            ops.conv(x, w, bias, geom, cout=cout, out=y, out_t=(2, par), res=res, res_mode=L.VT_RES_MIX, mix_factor=mf)
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all() and float(y[..., cout:].float().abs().max()) == 0
    for e in rec:
        plan, ar = _replay_check(e, "frame interleave")
        assert plan["tile"] == (128, 128) and ar.slots["y"].real_bytes + 16 == ar.slots["y"].row_bytes


# ---- the paired time up-sampler -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", T.H16, ids=T.H16_IDS)
@pytest.mark.parametrize("shape,C_,ln,ldv_pad", [((2, 3, 16, 16), 256, True, 0), ((1, 2, 16, 32), 512, False, 0), ((1, 1, 16, 16), 256, False, 0),
                                                 ((1, 2, 16, 48), 256, True, 0), ((1, 2, 16, 48), 256, False, 8)],
                         ids=["b2_ln", "two_channel_tiles", "single_frame", "768_pixel_frames_ln", "768_pixel_frames_ldv_pad"])
def test_time_upsample3(shape, C_, ln, ldv_pad, dtype, vt_opts):
    """the operator shapes of tests/test_gpu_time_upsample3.py, 16 x 48 frames (768 pixels: three tiles per frame, tile edges in mid-row),
    and V at ldv = C + 8"""
    vt_opts(conv_tile=256)
    x, _w, bias, wu, wv, mf, gam, bet = tup3_operands(*shape, C_, dtype)
    lnp = (gam, bet, 1e-6, True) if ln else None
    with recording() as rec:
        if ldv_pad:
            v = ops.conv(x, wv, None, ConvGeom(**T.G3), cout=C_, ldy=C_ + ldv_pad)
            y = torch.full((shape[0], 2 * shape[1]) + shape[2:] + (C_,), float("nan"), dtype=dtype, device=DEV)
            assert ops.time_upsample3(x, (wu, bias), v, mf, y, cout=C_) is not None, "vt_time_upsample3_supported refused a covered shape"
            torch.cuda.synchronize()
        else:
            y, n, v = tup3_run(x, bias, wu, wv, mf, lnp, C_)
    assert torch.isfinite(y.float()).all()
    assert len(rec) == 2 and isinstance(rec[1][0], ops.TimeUp3Desc) and rec[1][0].ldv == C_ + ldv_pad
    _replay_check(rec[0], "paired time up-sampler: V")
    plan, ar = _replay_check(rec[1], "paired time up-sampler")
    assert ar.slots["y"].owned is None and plan["ln_fused"] == ln


# ---- the fused temporal block ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", T.H16, ids=T.H16_IDS)
@pytest.mark.parametrize("shape,tmode,nxt,keep", T.TBLOCK_CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}" for c in T.TBLOCK_CASES])
def test_temporal_block(shape, tmode, nxt, keep, dt):
    x, ws, bs, norms = T._tblock_operands(shape, dt)
    next_ln = None if nxt is None else (norms[2][0], norms[2][1], nxt)
    assert ops.temporal_block_supported(x, tmode)
    with recording() as rec:
        ops.temporal_block(x, ws[0], bs[0], ws[1], bs[1], norms[0], norms[1], tmode=tmode, next_ln=next_ln, keep_y=keep)
    torch.cuda.synchronize()
    assert len(rec) == 1
    _, ar = _replay_check(rec[0], "temporal block (TBLOCK_CASES)")
    assert ("y" in ar.slots) == keep and ("n_out" in ar.slots) == (nxt is not None)


@pytest.mark.parametrize("dt", T.H16, ids=T.H16_IDS)
@pytest.mark.parametrize("shape,off,cuts", [((2, 14, 16, 16), 0, (5, 9)), ((1, 26, 64, 64), 4, (9, 17)), ((3, 12, 24, 48), 2, (6,))],
                         ids=["two_cuts", "lookahead_4_256_columns", "lookahead_2_uneven_split"])
def test_temporal_block_chunked(shape, off, cuts, dt):
    """the chunks of test_temporal_block_chunked: the cache slots are in/out -- they enter with the bytes from before the plain launch and
    must leave with the bytes the plain launch left (both frames of each cache are rewritten)"""
    B, Tt, H, W = shape
    x, ws, bs, norms = T._tblock_operands(shape, dt)
    nxt = (norms[2][0], norms[2][1], True)
    caches = tuple(torch.full((B, 2, H, W, 128), float("nan"), dtype=dt, device=DEV) for _ in range(2))
    bounds, start = [], 0
    for cpos in list(cuts) + [Tt]:
        bounds.append((start, cpos))
        start = cpos - off
    for i, (t0, t1) in enumerate(bounds):
        tmode = L.VT_TPAD_REPLICATE if i == 0 else L.VT_TPAD_CACHE
        xs = x[:, t0:t1].contiguous()
        assert ops.temporal_block_supported(xs, tmode, None, caches, off)
        before = {c.data_ptr(): c.clone() for c in caches}
        with recording() as rec:
            ops.temporal_block(xs, ws[0], bs[0], ws[1], bs[1], norms[0], norms[1], next_ln=nxt, tmode=tmode, caches=caches, cache_offset=off)
        torch.cuda.synchronize()
        assert len(rec) == 1 and all(torch.isfinite(c.float()).all() for c in caches)
        _, ar = _replay_check(rec[0], "temporal block, chunked", pre=before)
        assert ar.slots["cache1"].kind == ar.slots["cache2"].kind == "inout"


# ---- gemm_nt, flash attention -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("Z,M,N,K,bcast,use_bias", [(3, 80, 48, 128, False, False), (2, 512, 64, 512, True, True), (5, 16, 16, 16, False, False),
                                                      (2, 100, 512, 104, False, True)])
def test_gemm_nt(Z, M, N, K, bcast, use_bias, dtype):
    with recording() as rec:
        T.test_gemm_nt(Z, M, N, K, bcast, use_bias, dtype)
        a = T._rand((1 if bcast else Z, M, K), dtype, 1, 1.0 / math.sqrt(K))
        y = ops.gemm_nt(a, T._rand((Z, N, K), dtype, 2), ld_out=N + 8)               # ld_out > N: the columns N .. stay zero
    torch.cuda.synchronize()
    assert len(rec) == 3 and float(y[..., N:].float().abs().max()) == 0
    for e in rec:
        _, ar = _replay_check(e, "gemm_nt")
    assert ar.slots["y"].row_bytes == (N + 8) * y.element_size() and ar.slots["y"].real_bytes == N * y.element_size()


@pytest.mark.parametrize("Z,S,ld,use_bias", [(2, 64, 64, True), (3, 256, 256, False), (2, 128, 136, True)], ids=["one_q_tile", "s256", "padded_vT"])
@pytest.mark.parametrize("dt", T.H16, ids=T.H16_IDS)
def test_flash_attention(Z, S, ld, use_bias, dt):
    """the padding columns S .. ld-1 of V^T hold 0xFF, not zeros: the kernel walks S / 32 key tiles and must never see them"""
    C_ = 512
    q, k, v = (T._rand((Z, S, C_), dt, i) for i in (1, 2, 3))
    vT = torch.empty((Z, C_, ld), dtype=dt, device=DEV)
    vT.view(torch.uint8).fill_(0xFF)
    vT[:, :, :S] = v.transpose(1, 2)
    bias = T._rand((C_,), F32, 4, 0.3) if use_bias else None
    assert ops.flash_attention_supported(q, vT)
    with recording() as rec:
        o = ops.flash_attention(q, k, vT, bias, C_ ** -0.5)
    torch.cuda.synchronize()
    assert len(rec) == 1 and torch.isfinite(o.float()).all()
    _replay_check(rec[0], "flash attention")


# ---- operators without a launch record: the C calls of the plain ops.* run, replayed with arena pointers ------------------------------
def _direct(names, run, operands, scratch=None):
    """run(): the plain ops.* call(s); operands(result) -> the operand list of arena.relocate_calls"""
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
    COUNTS["direct: " + names[0]] += len(new)
    return ar


def _in(name, t):
    return dict(name=name, t=t)


def _out(name, t, **kw):
    return dict(name=name, t=t, kind="out", **kw)


def _frames(t, t0, n):
    """owned rows of [B, Td, ...] seen as rows of one frame: the frames t0 .. t0 + n - 1 of every clip"""
    m = torch.zeros(tuple(t.shape[:2]), dtype=torch.bool)
    m[:, t0:t0 + n] = True
    return dict(ld=t[0, 0].numel(), c=t[0, 0].numel(), owned=m)


def _padded(rows, c, ld, dtype, seed, scale=1.0, shift=0.0):
    x = torch.zeros((rows, ld), dtype=dtype)
    x[:, :c] = (torch.randn((rows, c), generator=torch.Generator().manual_seed(seed)) * scale + shift).to(dtype)
    return x.to(DEV)


@pytest.mark.parametrize("din,dout", [(BF16, BF16), (F32, F32), (F32, BF16)], ids=["bf16", "f32", "f32_to_bf16"])
@pytest.mark.parametrize("rows", [1, 5, 231])
@pytest.mark.parametrize("c", [32, 128, 192, 512])
def test_layernorm_act(c, rows, din, dout):
    x = _padded(rows, c, c + 8, din, 1, 2.0, 0.5)
    gm, bt = 1 + 0.1 * T._rand((c,), F32, 2), 0.1 * T._rand((c,), F32, 3)
    _direct(["vt_layernorm_act"], lambda: ops.layernorm_act(x, gm, bt, silu=True, out_dtype=dout, c=c),
            lambda y: [_in("x", x), _in("gamma", gm), _in("beta", bt), _out("y", y, ld=c + 8, c=c)])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_softmax_rows(dtype):
    s = T._rand((5, 33, 100), F32, 1, 8.0)
    _direct(["vt_softmax_rows"], lambda: ops.softmax_rows(s, 0.0442, dtype, ld_out=104), lambda p: [_in("s", s), _out("p", p, ld=104, c=100)])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_layout_conversions(dtype):
    x = T._rand((2, 3, 5, 6, 7), F32, 1)
    ar = _direct(["vt_ncthw_to_ndhwc"], lambda: ops.ncthw_to_ndhwc(x, dtype, tpad=3), lambda y: [_in("x", x), _out("y", y, ld=8, c=3)])
    y = ar.view("y", dtype, (2, 8, 6, 7, 8)).clone()
    assert float(y[..., 3:].float().abs().max()) == 0                      # this operator DEFINES its pad lanes: zero
    _direct(["vt_ndhwc_to_ncthw"], lambda: ops.ndhwc_to_ncthw(y, 3, ttrim=3), lambda z: [_in("x", y), _out("y", z)])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("tmode", [L.VT_TPAD_ZERO, L.VT_TPAD_REPLICATE, L.VT_TPAD_CACHE, L.VT_TPAD_ZERO_BACK])
def test_time_avgpool(tmode, dtype):
    x = T._act(2, 9, 4, 4, 128, dtype, 1)
    cache = T._act(2, 1, 4, 4, 128, dtype, 2) if tmode == L.VT_TPAD_CACHE else None
    _direct(["vt_time_avgpool3s2"], lambda: ops.time_avgpool3s2(x, tmode, cache),
            lambda y: [_in("x", x), _out("y", y)] + ([_in("cache", cache)] if cache is not None else []))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("Ti", [1, 5])
def test_time_lerp2x_into_a_frame_range(Ti, dtype):
    x = T._act(2, Ti, 4, 4, 128, dtype, 1)
    out = torch.zeros((2, 2 * Ti + 3, 4, 4, 128), dtype=dtype, device=DEV)
    ar = _direct(["vt_time_lerp2x"], lambda: ops.time_lerp2x(x, out=out, out_t0=2), lambda o: [_in("x", x), _out("out", o, **_frames(o, 2, 2 * Ti))])
    assert COUNTS["direct: vt_time_lerp2x"] >= 2 and ar.slots["out"].owned.numel() == 2 * (2 * Ti + 3)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("nh,Tt,skip", [(1, 4, 2), (2, 5, 4), (2, 1, 0), (1, 3, 7)])
def test_time_lerp2x_cat(nh, Tt, skip, dtype):
    head, x = T._act(2, nh, 4, 4, 128, dtype, 1), T._act(2, Tt, 4, 4, 128, dtype, 2)
    _direct(["vt_time_lerp2x_cat"], lambda: ops.time_lerp2x_cat(head, x, skip), lambda y: [_in("head", head), _in("x", x), _out("y", y)])


def test_gather_frames_into_a_frame_range():
    x = T._act(2, 5, 4, 4, 128, BF16, 1)
    out = torch.full((2, 9, 4, 4, 128), 3.0, dtype=BF16, device=DEV)
    _direct(["vt_gather_frames"], lambda: ops.gather_frames(x, [1, 4, 4], out=out, out_t0=3), lambda o: [_in("src", x), _out("out", o, **_frames(o, 3, 3))])
    xi = torch.arange(2 * 3 * 5, dtype=torch.int32, device=DEV).reshape(2, 3, 5)               # any [B, T, ...] tensor: 20-byte frames
    oi = torch.zeros((2, 7, 5), dtype=torch.int32, device=DEV)
    _direct(["vt_gather_frames"], lambda: ops.gather_frames(xi, [2, 0], out=oi, out_t0=4), lambda o: [_in("src", xi), _out("out", o, **_frames(o, 4, 2))])


GN_GATE = {F32: 2e-5, BF16: 1.2e-2}          # test_groupnorm_act's gates


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("scope", [L.VT_GN_FRAME, L.VT_GN_PIXEL, L.VT_GN_CLIP], ids=["frame", "pixel", "clip"])
def test_groupnorm_act(scope, dtype):
    """vt_groupnorm_act sums its statistics with fp64 atomics (not reproducible run to run): finite and inside the operator's gate against
    the plain run; `work` carved at exactly vt_groupnorm_work_bytes() and handed over as 0xFF"""
    B, Tt, H, W, C_ = 2, 5, 12, 10, 128
    x = T._act(B, Tt, H, W, C_, dtype, 1) * 1.5 + 0.3
    gam, bet = T._rand((C_,), F32, 2, 0.3) + 1.0, T._rand((C_,), F32, 3, 0.2)
    nb = L.load().vt_groupnorm_work_bytes(B, Tt, 32, scope)           # (0 for the pixel scope: a slot of no bytes between two moats)
    assert nb >= 0

    def gate(got, exp):
        g, e = got.view(dtype), exp.view(dtype)
        assert torch.isfinite(g.float()).all() and rel_err(g, e) < GN_GATE[dtype], rel_err(g, e)

    _direct(["vt_groupnorm_act"], lambda: ops.groupnorm_act(x, gam, bet, scope=scope, silu=True),
            lambda y: [_in("x", x), _in("gamma", gam), _in("beta", bet), _out("y", y, ld=C_, c=C_, compare=gate)], scratch={16: nb})


# ---- the decoder-gradient kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("with_acc", [False, True], ids=["plain", "acc"])
@pytest.mark.parametrize("gname,dims,cin,cout", [("3x3x3", (2, 3, 5, 6), 12, 20), ("3x3", (1, 2, 16, 16), 128, 128), ("k3", (1, 5, 8, 8), 128, 128),
                                                 ("3x3_fold", (1, 2, 8, 8), 128, 128)])
def test_conv_dgrad(gname, dims, cin, cout, with_acc, dtype):
    geom = {"3x3x3": ConvGeom(**T.G333), "3x3": ConvGeom(**T.G3), "k3": ConvGeom(kt=3, pt=2), "3x3_fold": ConvGeom(ups_s=1, **T.G3)}[gname]
    B, Ti, Hi, Wi = dims
    To, Ho, Wo = geom.out_dims(Ti, Hi, Wi)
    dy = T._act(B, To, Ho, Wo, cout, dtype, 1)
    gen = torch.Generator().manual_seed(2)
    w5 = torch.randn((cout, cin, geom.kt, geom.kh, geom.kw), generator=gen) / math.sqrt(cin * geom.kt * geom.kh * geom.kw)
    wt = ops.pack_conv_weight_dgrad(w5.to(DEV), dtype, dy.shape[-1])
    acc = T._act(B, Ti, Hi, Wi, cin, dtype, 3) if with_acc else None
    ldx = ops.pad_channels(cin)
    _direct(["vt_conv_dgrad"], lambda: ops.conv_dgrad(dy, wt, geom, cin=cin, cout=cout, acc=acc),
            lambda dx: [_in("dy", dy), _in("wt", wt), _out("dx", dx, ld=ldx, c=cin)] + ([_in("acc", acc)] if with_acc else []))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("c,ld,rows", [(100, 104, 231), (192, 192, 5), (4, 8, 33), (512, 512, 1)])
def test_layernorm_act_backward(c, ld, rows, dtype):
    """(the pad lanes of dx must lie within the 64-channel group above C: ld = C + 8 is not available for C = 128 or 512)"""
    y, dn = _padded(rows, c, ld, dtype, 1, 2.0, 0.5), _padded(rows, c, ld, dtype, 2)
    gm, bt = 1 + 0.1 * T._rand((c,), F32, 3), 0.1 * T._rand((c,), F32, 4)
    nb = L.load().vt_layernorm_act_backward_work_bytes(rows, c)
    assert nb >= 0
    _direct(["vt_layernorm_act_backward"], lambda: ops.layernorm_act_backward(y, dn, gm, bt, silu=True, c=c),
            lambda r: [_in("y", y), _in("dn", dn), _in("gamma", gm), _in("beta", bt), _out("dx", r[0], ld=ld, c=c), _out("dgamma", r[1]), _out("dbeta", r[2])],
            scratch={15: nb})


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_grad_fold(dtype):
    B, Tt, H, W, c, ld, rep = 2, 3, 4, 5, 20, 24, 1
    src = T._act(B, rep + 2 * Tt, 2 * H, 2 * W, c, F32, 1)
    acc = T._act(B, Tt, H, W, c, dtype, 2)
    _direct(["vt_grad_fold"], lambda: ops.grad_fold(src, ups_t=1, ups_s=1, rep=rep, c=c, acc=acc, out_dtype=dtype),
            lambda o: [_in("src", src), _in("acc", acc), _out("out", o, ld=ld, c=c)])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_softmax_rows_backward(dtype):
    s = T._rand((3, 30, 30), F32, 1, 4.0)
    p = ops.softmax_rows(s, 512 ** -0.5, dtype, ld_out=32)
    dp = T._rand((3, 30, 30), F32, 2)
    _direct(["vt_softmax_rows_backward"], lambda: ops.softmax_rows_backward(p, dp, 512 ** -0.5, cols=30, ld_out=32),
            lambda ds: [_in("p", p), _in("dp", dp), _out("ds", ds, ld=32, c=30)])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_transpose_batched(dtype):
    x = T._rand((5, 30, 40), dtype, 2)
    _direct(["vt_transpose_batched"], lambda: ops.transpose_batched(x, cols=36, ld_out=32), lambda t: [_in("x", x), _out("out", t, ld=32, c=30)])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_upsample_mix_forward_backward(dtype):
    shape, ch = (2, 6, 7, 9, 24), 20
    u, c, dy = (T._rand(shape, dtype, i) + 1.0 for i in (1, 2, 3))
    mf = torch.tensor([0.37], device=DEV)
    _direct(["vt_upsample_mix"], lambda: ops.upsample_mix(u, c, mf, ch=ch), lambda y: [_in("u", u), _in("c", c), _in("mix", mf), _out("y", y, ld=24, c=ch)])
    M = dy.numel() // 24
    nb = L.load().vt_upsample_mix_backward_work_bytes(M, 24)
    _direct(["vt_upsample_mix_backward"], lambda: ops.upsample_mix_backward(dy, u, c, mf, ch=ch),
            lambda r: [_in("dy", dy), _in("u", u), _in("c", c), _in("mix", mf), _out("du", r[0], ld=24, c=ch), _out("dc", r[1], ld=24, c=ch), _out("dmix", r[2])],
            scratch={11: nb})


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("Ti", [1, 5])
def test_time_lerp2x_backward(Ti, dtype):
    dy = T._rand((2, 2 * Ti + 3, 4, 5, 8), dtype, 6)
    out = torch.zeros((2, Ti + 1, 4, 5, 8), dtype=dtype, device=DEV)
    _direct(["vt_time_lerp2x_backward"], lambda: ops.time_lerp2x_backward(dy, 2, Ti, out, 1), lambda o: [_in("dy", dy), _out("out", o, **_frames(o, 1, Ti))])


# ---- what was reached (keep last) ---------------------------------------------------------------------------------------------------
def test_coverage_of_the_relocated_launches():
    """every kernel family of the issue was relocated at least once in this run of the file"""
    for fam in sorted(COUNTS):
        print(f"[arena] {fam}: {COUNTS[fam]} launches relocated")
    for key in sorted(REACHED, key=str):
        print(f"[arena] reached {key}")
    convs = [k for k in REACHED if len(k) == 5]
    has = lambda **kw: any(all(dict(kernel=k[0], tile=k[1], lds=k[2], deep=k[3], multi=k[4])[n] == v for n, v in kw.items()) for k in convs)      # noqa: E731
    want = {
        "igemm 128x128 with the LDS epilogue": has(kernel="igemm", tile=(128, 128), lds=True),
        "igemm 128x128 without the LDS epilogue": has(kernel="igemm", tile=(128, 128), lds=False, deep=False),
        "256x256 with the LDS epilogue": has(kernel="igemm", tile=(256, 256), lds=True),
        "256x256 without the LDS epilogue": has(kernel="igemm", tile=(256, 256), lds=False),
        "ws2": has(kernel="ws2"),
        "narrow": has(kernel="narrow"),
        "in8": has(kernel="in8"),
        "a split-K launch": COUNTS["split-K (SPLITK_CASES)"] > 0 and has(kernel="igemm", multi=True),
        "a deep ring": has(deep=True),
        "a paired launch": ("paired",) in REACHED,
        "a TBlockDesc": ("tblock",) in REACHED,
        "a flash launch": ("flash",) in REACHED,
    }
    missing = [k for k, v in want.items() if not v]
    assert not missing, f"not reached: {missing}"
