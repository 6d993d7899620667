"""The deterministic sweep of vt_conv descriptors behind tests/golden/conv_plan_table.json (scripts/make_golden_conv_plan.py records it,
tests/test_conv_plan_table.py replays it): what vt_conv_plan and vt_conv_work_bytes answer is a pure function of the descriptor and the
option table, needs no GPU (256 CUs assumed) and must not move when the selection code is reorganised.

The sweep = BASES (every layer class of DESIGN.md section 0's table at B = 4, 17 x 256 x 256 -- 20 / 10 / 5 frames per level --, the v1.1
chunk shapes, the small shapes of the GPU parity tests, descriptors the validation rejects) x the four arithmetic modes x MODS (LayerNorm
modes, ln_keep_y, residual modes, output layout) x OPTION_SETTINGS x {work = NULL, work = an aligned stand-in}.
"""
import ctypes as C
import hashlib

from vidtok_amd import lib as L

PTR = 1 << 20          # stand-in tensor address: 16-byte aligned, never dereferenced (nothing is launched)
WORK_BYTES = 1 << 40   # the stand-in scratch is large enough for every descriptor of the sweep

OPTION_SETTINGS = [{}, {"conv_tile": 128}, {"conv_tile": 256}] + [{n: 0} for n in (
    "conv_ws", "conv_narrow", "conv_in8", "conv_ldsepi", "conv_fuse_ln", "conv_fuse_ln256", "conv_tup_ln", "conv_deep", "conv_splitk", "conv_buf")]

MODES = ("bf16", "fp16", "fp32", "bf16x3")


def g(B, T, H, W, cin, cout, k=(1, 3, 3), **kw):
    """a stride-1 'same' convolution, causal in time (pt = kt - 1), on [B][T][H][W][cin]; keywords override descriptor fields"""
    kt, kh, kw_ = k
    d = dict(x=PTR, w=PTR, y=PTR, bias=PTR, B=B, Ti=T, Hi=H, Wi=W, Cin=cin, To=T, Ho=H, Wo=W, Cout=cout,
             ldw=kt * kh * kw_ * cin, ldy=cout, KT=kt, KH=kh, KW=kw_, st=1, sh=1, sw=1, pt=kt - 1, ph=kh // 2, pw=kw_ // 2, ln_eps=1e-6)
    d.update(kw)
    return d


CACHE = dict(tmode=L.VT_TPAD_CACHE, ncache=2, cache=PTR)

BASES = [
    # ---- DESIGN.md section 0, B = 4 clips of 17 x 256 x 256 ----
    g(4, 20, 256, 256, 128, 128),                                   # 3x3, Cin 128: the weight-stationary kernel
    g(4, 10, 256, 256, 512, 256),                                   # 3x3, Cin 512 -> 256, K = 4 608
    g(4, 10, 256, 256, 256, 256, (2, 3, 3), yt_mul=2, yt_off=1),     # time up-sampler parity 2x3x3, Cin 256
    g(4, 20, 128, 128, 256, 256), g(4, 10, 128, 128, 256, 256), g(4, 5, 128, 128, 256, 256),
    g(4, 5, 128, 128, 512, 512, (2, 3, 3), yt_mul=2, yt_off=0),      # time up-sampler parity 2x3x3, Cin 512
    g(4, 20, 256, 256, 256, 128),                                   # 3x3, Cin 256 -> 128
    g(4, 20, 128, 128, 256, 256, (3, 1, 1)), g(4, 10, 128, 128, 256, 256, (3, 1, 1)),     # temporal k = 3, Cin 256
    g(4, 5, 32, 32, 512, 512, (3, 3, 3)),                           # 3x3x3, Cin 512, M = 20 480
    g(4, 5, 64, 64, 512, 512), g(4, 10, 64, 64, 512, 512), g(4, 5, 32, 32, 512, 512),      # 3x3, Cin 512
    g(4, 10, 128, 128, 512, 256, (2, 1, 1), yt_mul=2, yt_off=1),     # time up-sampler parity k = 2
    g(4, 10, 128, 128, 256, 256, (1, 2, 2), ph=0, pw=0, ys_mul=2, ys_oh=1, ys_ow=0),      # space up-sampler parity 2x2, Cin 256
    g(4, 5, 64, 64, 512, 512, (1, 2, 2), ph=0, pw=0, ys_mul=2, ys_oh=0, ys_ow=1),         # ... Cin 512
    g(4, 20, 256, 256, 256, 128, (1, 1, 1)), g(4, 10, 128, 128, 512, 256, (1, 1, 1)), g(4, 5, 32, 32, 512, 512, (1, 1, 1)),   # 1x1
    g(4, 10, 64, 64, 512, 512, (3, 1, 1)), g(4, 5, 64, 64, 512, 512, (3, 1, 1)), g(4, 5, 32, 32, 512, 512, (3, 1, 1)),       # temporal, Cin 512
    g(4, 20, 256, 256, 8, 128, (3, 3, 3)),                          # conv_in: 3 channels stored as 8
    g(4, 20, 128, 128, 128, 256),                                   # 3x3, Cin 128 -> 256
    g(4, 20, 256, 256, 128, 128, Ho=128, Wo=128, sh=2, sw=2, ph=0, pw=0),                 # the stride-2 down-sampler
    g(4, 20, 256, 256, 128, 128, (3, 1, 1), To=10, st=2),           # ... in time
    g(4, 10, 64, 64, 256, 256, (3, 3, 3)), g(4, 10, 64, 64, 256, 512),
    g(4, 5, 32, 32, 512, 8, (3, 3, 3)),                             # the encoder's conv_out
    g(4, 20, 256, 256, 128, 3, (3, 3, 3), ldy=4, t_trim=3),         # the decoder's conv_out (narrow kernel with NCTHW output)
    g(1, 1, 32, 32, 512, 1024, (1, 1, 1), nbatch=20, xs_z=1024 * 512, ws_z=1024 * 512, ys_z=1024 * 1024),   # attention: Q K^T per frame
    g(1, 1, 32, 32, 1024, 512, (1, 1, 1), nbatch=20, xs_z=1024 * 1024, ws_z=512 * 1024, ys_z=1024 * 512),   # ... P V
    # ---- v1.1 chunks (B = 1; frames before the chunk from the cache, or the first frame replicated) ----
    g(1, 4, 32, 32, 512, 512, (3, 3, 3), **CACHE), g(1, 5, 32, 32, 512, 512, (3, 3, 3), **CACHE), g(1, 4, 32, 32, 512, 512),
    g(1, 4, 32, 32, 512, 512, (3, 1, 1), **CACHE), g(1, 8, 64, 64, 256, 256, (3, 3, 3), **CACHE), g(1, 8, 24, 24, 512, 512, (3, 3, 3), **CACHE),
    g(1, 16, 256, 256, 128, 128), g(1, 16, 256, 256, 8, 128, (3, 3, 3), tmode=L.VT_TPAD_REPLICATE),
    g(1, 16, 256, 256, 128, 3, (3, 3, 3), ldy=4, **CACHE), g(1, 16, 128, 128, 256, 256, (3, 1, 1), tmode=L.VT_TPAD_REPLICATE),
    # ---- small shapes of the GPU parity tests ----
    g(1, 1, 64, 64, 256, 256), g(1, 1, 64, 64, 128, 128), g(1, 1, 64, 64, 512, 512), g(2, 3, 16, 16, 64, 128, (3, 3, 3)),
    g(1, 4, 16, 16, 256, 128, (3, 3, 3)), g(1, 4, 16, 16, 256, 256, (3, 3, 3)), g(1, 2, 24, 20, 24, 96), g(1, 3, 17, 19, 40, 200),
    g(1, 1, 64, 64, 128, 8), g(1, 1, 64, 64, 128, 64), g(1, 2, 32, 32, 32, 256, (3, 1, 1)), g(2, 5, 16, 16, 8, 128, (3, 3, 3)),
    g(1, 3, 16, 28, 128, 3, (3, 3, 3), ldy=4), g(1, 2, 16, 16, 128, 128, Hi=8, Wi=8, ups_s=1), g(1, 4, 16, 16, 128, 256, (3, 1, 1), Ti=2, ups_t=1),
    g(1, 2, 16, 16, 256, 256, ldy=260), g(1, 2, 16, 16, 256, 256, (1, 1, 1), nbatch=3, xs_z=512 * 256, ws_z=0, ys_z=512 * 256),
    # ---- rejected by the validation ----
    g(1, 1, 64, 64, 100, 128), g(1, 1, 64, 64, 128, 128, x=0), g(1, 1, 64, 64, 128, 128, x=PTR + 4), g(1, 1, 64, 64, 128, 128, ldy=64),
    g(1, 1, 64, 64, 128, 128, ys_mul=3), g(1, 2, 16, 16, 128, 128, yt_mul=2, yt_off=2), g(1, 2, 16, 16, 128, 128, nbatch=2, yt_mul=2),
    g(4096, 20, 256, 256, 128, 128), g(1, 2, 16, 16, 128, 128, (3, 3, 3), tmode=L.VT_TPAD_CACHE, ncache=1, cache=PTR),
    g(1, 2, 16, 16, 128, 128, (5, 5, 5)), g(1, 2, 16, 16, 128, 128, tmode=7), g(1, 2, 16, 16, 128, 128, ldw=1000),
]

LN = dict(ln_gamma=PTR, ln_beta=PTR, ln_out=PTR)
MODS = [
    {},
    dict(LN, ln_mode=1, ln_keep_y=0), dict(LN, ln_mode=1, ln_keep_y=1), dict(LN, ln_mode=2, ln_keep_y=0), dict(LN, ln_mode=2, ln_keep_y=1),
    dict(res_mode=L.VT_RES_ADD, res=PTR), dict(res_mode=L.VT_RES_MIX, res=PTR, mix_factor=PTR),
    dict(LN, ln_mode=2, ln_keep_y=1, res_mode=L.VT_RES_ADD, res=PTR), dict(LN, ln_mode=1, ln_keep_y=0, res_mode=L.VT_RES_MIX, res=PTR, mix_factor=PTR),
    dict(res_mode=L.VT_RES_ADD, res=PTR, res_tshift=1),      # the residual of a time up-sampler: one frame for two
    dict(out_layout=L.VT_NCTHW),                            # fp32 results in the reference's layout
    dict(LN, ln_mode=3), dict(res_mode=L.VT_RES_ADD),       # rejected: no such mode, no operand
]


def make_desc(base, mode, mod, work):
    f = dict(base)
    f.update(mod)
    dt = {"bf16": L.VT_BF16, "fp16": L.VT_F16, "fp32": L.VT_F32, "bf16x3": L.VT_BF16X3}[mode]
    f["dtype"] = dt
    f["out_dtype"] = L.VT_F32 if (mode == "bf16x3" or f.get("out_layout") == L.VT_NCTHW) else dt
    if mode == "bf16x3":
        f["ldw"] = (f["ldw"] + 31) // 32 * 32                # the split weight planes pad K to the block
    if "ln_mode" in f:
        f.setdefault("ldn", f["ldy"])
    if f.get("res_mode"):
        f.setdefault("ldr", f["ldy"])
        f.setdefault("Tr", (f["To"] + 1) // 2 if f.get("res_tshift") else f["To"])
    if work:
        f["work"], f["work_bytes"] = PTR, WORK_BYTES
    d = L.ConvDesc()
    for k, v in f.items():
        setattr(d, k, v)
    return d


def cases():
    """(option setting, descriptor) in the table's row order"""
    for opts in OPTION_SETTINGS:
        for base in BASES:
            for mode in MODES:
                for mod in MODS:
                    for work in (False, True):
                        yield opts, make_desc(base, mode, mod, work)


def run_sweep(lib):
    """-> (rows, digest, reached): per case [rc, out8[0..7], work_bytes] of vt_conv_plan / vt_conv_work_bytes, a digest of the descriptors
    asked, and the names of REQUIRED the sweep reached"""
    rows, h, cur, reached = [], hashlib.sha256(), None, set()
    lib.vt_reset_options()
    try:
        for opts, d in cases():
            if opts is not cur:
                lib.vt_reset_options()
                for k, v in opts.items():
                    L.check(lib.vt_set_option(k.encode(), v), k)
                cur = opts
                h.update(repr(sorted(opts.items())).encode())
            h.update(bytes(d))
            out = (C.c_int32 * 8)()
            rc = lib.vt_conv_plan(C.byref(d), out)
            rows.append([rc] + (list(out) if rc == 0 else [0] * 8) + [lib.vt_conv_work_bytes(C.byref(d))])
            if rc == 0:
                reached.update(n for n, hit in REQUIRED.items() if n not in reached and hit(signature(rows[-1]), rows[-1][9], d))
    finally:
        lib.vt_reset_options()
    return rows, h.hexdigest(), reached


def signature(row):
    """(kernel, pixel tile, channel tile, LayerNorm fused, launches, epilogue / ring form) of an accepted row"""
    return (row[7], row[1], row[2], row[5], row[6], row[8])


# what the sweep has to reach, as predicates over (signature, work_bytes, descriptor): a table without one of these is too thin to pin the selection
REQUIRED = {
    "igemm kernel": lambda s, wb, d: s[0] == 0, "narrow kernel": lambda s, wb, d: s[0] == 2,
    "ws2 kernel": lambda s, wb, d: s[0] == 3, "in8 kernel": lambda s, wb, d: s[0] == 4,
    "tile 256x32": lambda s, wb, d: s[:3] == (0, 256, 32), "tile 256x64": lambda s, wb, d: s[:3] == (0, 256, 64),
    "tile 256x256": lambda s, wb, d: s[:3] == (0, 256, 256), "tile 128x128": lambda s, wb, d: s[:3] == (0, 128, 128),
    "LayerNorm fused in the 128-tile": lambda s, wb, d: s[:4] == (0, 128, 128, 1),
    "LayerNorm fused in the 256-tile": lambda s, wb, d: s[:4] == (0, 256, 256, 1) and s[5] == 1,
    "alpha-mix + LayerNorm fused in the 256-tile": lambda s, wb, d: s[:4] == (0, 256, 256, 1) and d.res_mode == L.VT_RES_MIX,
    "LayerNorm fused in ws2": lambda s, wb, d: s[0] == 3 and s[3] == 1, "LayerNorm fused in in8": lambda s, wb, d: s[0] == 4 and s[3] == 1,
    "plain LDS epilogue": lambda s, wb, d: s[:4] == (0, 256, 256, 0) and s[5] == 1,
    "vector epilogue on the 256-tile": lambda s, wb, d: s[:3] == (0, 256, 256) and s[5] == 0,
    "deep ring": lambda s, wb, d: s[5] == 2,
    "split-K by time taps": lambda s, wb, d: s[0] == 0 and s[4] == 2 and wb > 0 and bool(d.work) and d.KT == 3,
    "split-K by rows": lambda s, wb, d: s[0] == 0 and s[4] == 2 and wb > 0 and bool(d.work) and d.KT == 1 and d.KH == 3,
    "split-K in cache mode": lambda s, wb, d: wb > 0 and d.tmode == L.VT_TPAD_CACHE,
    "split-K + separate LayerNorm": lambda s, wb, d: s[4] == 3,
    "two-pass narrow launch": lambda s, wb, d: s[0] == 2 and s[4] == 2,
    "two launches: un-fused LayerNorm": lambda s, wb, d: s[0] == 0 and s[4] == 2 and wb == 0 and d.ln_mode != 0,
    "batched GEMM (nbatch > 1)": lambda s, wb, d: d.nbatch > 1,
    "frame interleave": lambda s, wb, d: d.yt_mul == 2, "pixel interleave": lambda s, wb, d: d.ys_mul == 2,
    "NCTHW output": lambda s, wb, d: d.out_layout == L.VT_NCTHW,
}
