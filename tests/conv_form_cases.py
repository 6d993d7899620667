"""The sweep behind tests/golden/conv_launch_form_table.json (scripts/make_golden_conv_plan.py --form records it,
tests/test_conv_form_table.py replays it): what vt_conv_launch_form answers -- the gather form, the descriptor extents, the skipped time
taps, the tile order, the K steps, the schedule and the LDS of the implicit-GEMM launch behind vt_conv, vt_time_upsample3 and vt_conv_act --
is a pure function of the descriptor and the option table, needs no GPU and must not move when the launch code is reorganised.  None of
these choices changes a result bit, so no parity test sees them; this table does.

The sweep = the descriptors of tests/conv_plan_cases.py, under its option settings plus the two it lacks (conv_tskip = 0, conv_tinner = 0),
asked for each of the three calls.
"""
import ctypes as C
import hashlib

import conv_plan_cases as S
from vidtok_amd import lib as L

OPTION_SETTINGS = S.OPTION_SETTINGS + [{"conv_tskip": 0}, {"conv_tinner": 0}]
CALLS = (0, 1, 2)      # vt_conv, vt_time_upsample3, vt_conv_act with ReLU
# out16 of vt_conv_launch_form (include/vidtok_amd.h)
KERNEL, BUF, X_BYTES, W_BYTES, C_BYTES, TSKIP, HW_TILES, LDS_EPI, NSTEPS, M_TILES, N_TILES, GRID_Z, KSPLIT, SCHED, LDS_BYTES, VARIANT = range(16)
TILE_256x256, TILE_128x128 = 2, 3


def cases():
    """(option setting, call, descriptor) in the table's row order"""
    for opts in OPTION_SETTINGS:
        for call in CALLS:
            for base in S.BASES:
                for mode in S.MODES:
                    for mod in S.MODS:
                        for work in (False, True):
                            yield opts, call, S.make_desc(base, mode, mod, work)


def run_sweep(lib):
    """-> (rows, digest, reached): per case [rc, call, out16[0..15]] (zeros where rejected), a digest of what was asked, and the names of
    REQUIRED the sweep reached"""
    rows, h, cur, reached = [], hashlib.sha256(), None, set()
    lib.vt_reset_options()
    try:
        for opts, call, d in cases():
            if opts is not cur:
                lib.vt_reset_options()
                for k, v in opts.items():
                    L.check(lib.vt_set_option(k.encode(), v), k)
                cur = opts
                h.update(repr(sorted(opts.items())).encode())
            h.update(bytes(d) + bytes([call]))
            out = (C.c_int64 * 16)()
            rc = lib.vt_conv_launch_form(C.byref(d), call, out)
            rows.append([rc, call] + (list(out) if rc == 0 else [0] * 16))
            if rc == 0 and out[KERNEL] == 0:
                reached.update(n for n, hit in REQUIRED.items() if n not in reached and hit(call, out, d) and (n not in BY_ITSELF or "conv_buf" not in opts))
    finally:
        lib.vt_reset_options()
    return rows, h.hexdigest(), reached


def tile(out):
    return out[VARIANT] & 15


# reached only by a row recorded with option conv_buf on: the launch fell back to pointers by itself
BY_ITSELF = ("pointer gather", "cache mode on pointers (24 x 24: a tile spans frames)")
# what the sweep has to reach, as predicates over (call, out16 of an accepted implicit-GEMM row, descriptor)
REQUIRED = {
    "descriptor gather": lambda c, o, d: o[BUF] == 1 and o[X_BYTES] > 0 and o[W_BYTES] > 0,
    "pointer gather": lambda c, o, d: o[BUF] == 0 and o[X_BYTES] == 0,
    "cache mode on descriptors": lambda c, o, d: d.tmode == L.VT_TPAD_CACHE and d.pt > 0 and o[BUF] == 1 and o[C_BYTES] > 0,
    "cache mode on pointers (24 x 24: a tile spans frames)": lambda c, o, d: d.tmode == L.VT_TPAD_CACHE and d.Ho == 24 and o[BUF] == 0,
    "time taps skipped": lambda c, o, d: c == 0 and o[TSKIP] == 1,
    "time taps not skipped on a temporal convolution": lambda c, o, d: c == 0 and o[TSKIP] == 0 and d.KT > 1 and d.pt > 0,
    "frames innermost on the 256-pixel tile": lambda c, o, d: o[HW_TILES] > 0 and tile(o) == TILE_256x256,
    "frames innermost on the 128-pixel tile": lambda c, o, d: o[HW_TILES] > 0 and tile(o) == TILE_128x128,
    "pixel order on a temporal convolution": lambda c, o, d: o[HW_TILES] == 0 and d.KT > 1 and d.To > 1,
    "128-tile with the LDS epilogue": lambda c, o, d: tile(o) == TILE_128x128 and o[LDS_EPI] == 1,
    "128-tile without the LDS epilogue": lambda c, o, d: tile(o) == TILE_128x128 and o[LDS_EPI] == 0,
    "schedule 0": lambda c, o, d: o[SCHED] == 0, "schedule 1": lambda c, o, d: o[SCHED] == 1,
    "schedule 2": lambda c, o, d: o[SCHED] == 2, "schedule 5": lambda c, o, d: o[SCHED] == 5,
    "split partial launch by time taps": lambda c, o, d: c == 0 and o[KSPLIT] == 1 and o[GRID_Z] == 3 and d.KT == 3,
    "split partial launch by rows": lambda c, o, d: c == 0 and o[KSPLIT] == 2 and o[GRID_Z] == 3 and d.KT == 1 and d.KH == 3,
    "paired launch with skipped taps": lambda c, o, d: c == 1 and o[TSKIP] == 1 and (o[VARIANT] >> 8 & 15) == 2,
    "ReLU launch": lambda c, o, d: c == 2,
}
