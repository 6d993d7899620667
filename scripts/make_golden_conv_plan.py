"""Record what vt_conv_plan and vt_conv_work_bytes answer on the sweep of tests/conv_plan_cases.py -> tests/golden/conv_plan_table.json
(tests/test_conv_plan_table.py replays it against the built library, row for row; no GPU needed).

    python scripts/make_golden_conv_plan.py [--lib PATH] [--out PATH]     record (default: the in-tree library, the committed table)
    python scripts/make_golden_conv_plan.py --form [--lib PATH] [--out PATH]   record vt_conv_launch_form on the sweep of tests/conv_form_cases.py
                                                                          -> tests/golden/conv_launch_form_table.json (tests/test_conv_form_table.py)
    python scripts/make_golden_conv_plan.py --time [--lib PATH]           time 100 000 vt_conv_plan calls over a handful of the descriptors

The table pins the selection, so it is recorded with the library of the commit BEFORE a change of the selection code.  Only the answers
are stored: `unique` lists the distinct [rc, out8[0..7], work_bytes] rows, `rows` run-length encodes the index of every case's answer
([index, repeats]), `digest` identifies the descriptors asked, `signatures` the distinct (kernel, tile, LayerNorm fused, launches,
epilogue / ring form) that occur.  The form table has the same encoding with rows [rc, call, out16[0..15]] and no signatures; its first
recording came from a build of the commit before vt_conv_launch_form existed, patched to note what its launch code computed right before
each launch and to launch nothing.  A row that differs later is a finding about the change at hand, never a reason to record again."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conv_plan_cases as S  # noqa: E402
from util import GOLDEN_DIR  # noqa: E402
from vidtok_amd import lib as L  # noqa: E402


def encode(rows):
    unique = sorted({tuple(r) for r in rows})
    index = {r: i for i, r in enumerate(unique)}
    runs = []
    for r in rows:
        i = index[tuple(r)]
        if runs and runs[-1][0] == i:
            runs[-1][1] += 1
        else:
            runs.append([i, 1])
    return [list(r) for r in unique], runs


def decode(table):
    return [table["unique"][i] for i, n in table["rows"] for _ in range(n)]


def signatures(rows):
    return sorted({S.signature(r) for r in rows if r[0] == 0})


def time_plan(lib, calls=100_000):
    import ctypes as C
    descs = [S.make_desc(S.BASES[i], mode, S.MODS[m], work) for i, mode, m, work in
             ((0, "bf16", 3, False), (1, "bf16", 4, False), (10, "bf16", 0, True), (23, "fp16", 3, False), (31, "bf16", 10, False), (6, "bf16x3", 6, False))]
    refs, out = [C.byref(d) for d in descs], (C.c_int32 * 8)()
    plan, n = lib.vt_conv_plan, len(descs)
    t0 = time.perf_counter()
    for i in range(calls):
        plan(refs[i % n], out)
    return (time.perf_counter() - t0) / calls * 1e9


def record_form(lib, out):
    import conv_form_cases as F
    rows, digest, reached = F.run_sweep(lib)
    missing = sorted(set(F.REQUIRED) - reached)
    print(f"{len(rows)} cases, {sum(r[0] != 0 for r in rows)} rejected, {sum(r[0] == 0 and r[2] == 0 for r in rows)} implicit-GEMM launches")
    if missing:
        print("the sweep does not reach:", ", ".join(missing))
        return 1
    unique, runs = encode(rows)
    with open(out, "w") as f:
        json.dump({"digest": digest, "cases": len(rows), "unique": unique, "rows": runs}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{out}: {len(unique)} distinct answers, {len(runs)} runs, {os.path.getsize(out)} bytes")
    return 0


def main(argv):
    lib = L.load(argv[argv.index("--lib") + 1] if "--lib" in argv else None)
    if "--form" in argv:
        return record_form(lib, argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(GOLDEN_DIR, "conv_launch_form_table.json"))
    if "--time" in argv:
        print("vt_conv_plan: " + ", ".join(f"{time_plan(lib):.0f}" for _ in range(3)) + " ns per call (three runs of 100 000, ctypes overhead included)")
        return 0
    rows, digest, reached = S.run_sweep(lib)
    missing = sorted(set(S.REQUIRED) - reached)
    sigs = signatures(rows)
    print(f"{len(rows)} cases, {sum(r[0] != 0 for r in rows)} rejected, {len(sigs)} distinct (kernel, tile, ln_fused, launches, form):")
    for s in sigs:
        print("  ", s)
    if missing:
        print("the sweep does not reach:", ", ".join(missing))
        return 1
    unique, runs = encode(rows)
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(GOLDEN_DIR, "conv_plan_table.json")
    with open(out, "w") as f:
        json.dump({"digest": digest, "cases": len(rows), "signatures": [list(s) for s in sigs], "unique": unique, "rows": runs}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{out}: {len(unique)} distinct answers, {len(runs)} runs, {os.path.getsize(out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
