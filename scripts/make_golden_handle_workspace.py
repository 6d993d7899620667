"""Record what the model handle's dry walks answer -> tests/golden/handle_workspace_table.json (tests/test_handle_workspace_table.py
replays it against the built library, integer for integer; no GPU needed).

    python scripts/make_golden_handle_workspace.py [--lib PATH] [--out PATH]     record (default: the in-tree library, the committed table)

vt_workspace_bytes and vt_tile_workspace_bytes walk both stage graphs of csrc/model.cpp dry: every allocation of every stage, the
split-K scratch the library asks for, the temporaries of the chunk caches and the twins allocated only after a probe said yes all end
in the arenas' peaks.  The table therefore pins the allocation order of the host graph, and it is recorded with the library of the
commit BEFORE a change of that file.  Rows: every YAML under configs/ x {VT_BF16, VT_F16, VT_F32, VT_BF16X3}, vt_workspace_bytes at
(1, T0, 64, 64) and (2, T0, 128, 96) with T0 = 2 f + 1 (causal) or 2 f (non-causal); for the v1.1 configs also
vt_tile_workspace_bytes at (1, 21, 64, 64) with t_chunk_enc 8, overlap 1 and 0, and at (1, 41, 64, 64) with t_chunk_enc 16, overlap 1;
and one v1.1 config once more with `norm_type: groupnorm` and with `interpolation_mode: nearest`.  A row that differs later is a
finding about the change at hand, never a reason to record again."""
import ctypes as C
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from util import CONFIG_DIR, GOLDEN_DIR, handle_config  # noqa: E402

DTYPES = ("VT_BF16", "VT_F16", "VT_F32", "VT_BF16X3")
VARIANTS = (("vidtok_v1_1/vidtok_kl_causal_488_4chn_v1_1", dict(norm_type="groupnorm")),
            ("vidtok_v1_1/vidtok_kl_causal_488_4chn_v1_1", dict(interpolation_mode="nearest")))
TILE_CASES = ((1, 21, 64, 64, 8, 1), (1, 21, 64, 64, 8, 0), (1, 41, 64, 64, 16, 1))


def config_names():
    paths = sorted(glob.glob(os.path.join(CONFIG_DIR, "*.yaml")) + glob.glob(os.path.join(CONFIG_DIR, "vidtok_v1_1", "*.yaml")))
    return [os.path.relpath(q, CONFIG_DIR)[:-5] for q in paths]


def run_table(lib):
    """{"<config>[+override]/<dtype>/<entry>(args)": bytes} of the library `lib` (vidtok_amd.lib.load)"""
    import vidtok_amd
    from vidtok_amd import lib as L

    rows = {}
    for name, ov in [(n, {}) for n in config_names()] + list(VARIANTS):
        prm = vidtok_amd.load_config(os.path.join(CONFIG_DIR, name + ".yaml"))["model"]["params"]
        enc, reg = dict(prm["encoder_config"]["params"], **ov), prm["regularizer_config"]
        mc = handle_config(L, enc, reg["target"], reg.get("params", {}), prm["encoder_config"]["target"])
        f = mc.time_downsample_factor
        t0 = 2 * f if mc.version == 2 else 2 * f + 1
        label = name + "".join(f"+{k}={v}" for k, v in ov.items())
        for dt in DTYPES:
            h = C.c_void_p()
            assert lib.vt_create(C.byref(mc), getattr(L, dt), C.byref(h)) == 0, lib.vt_last_error()
            try:
                for B, T, H, W in ((1, t0, 64, 64), (2, t0, 128, 96)):
                    rows[f"{label}/{dt}/workspace({B},{T},{H},{W})"] = lib.vt_workspace_bytes(h, B, T, H, W)
                for case in TILE_CASES if mc.version == 1 else ():
                    rows[f"{label}/{dt}/tile_workspace({','.join(map(str, case))})"] = lib.vt_tile_workspace_bytes(h, *case)
            finally:
                lib.vt_destroy(h)
    return rows


def main(argv):
    from vidtok_amd import lib as L

    rows = run_table(L.load(argv[argv.index("--lib") + 1] if "--lib" in argv else None))
    bad = [k for k, v in rows.items() if v <= 0]
    if bad:
        print("calls that failed:", ", ".join(bad))
        return 1
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(GOLDEN_DIR, "handle_workspace_table.json")
    with open(out, "w") as f:
        json.dump(rows, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{out}: {len(rows)} rows, {len(set(rows.values()))} distinct values, {os.path.getsize(out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
