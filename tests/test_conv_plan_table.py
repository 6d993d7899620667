"""vt_conv_plan / vt_conv_work_bytes against the recorded table (no GPU): the selection of kernel, tile, epilogue, ring and split-K for
every descriptor of the sweep (tests/conv_plan_cases.py) is exactly what the library answered when tests/golden/conv_plan_table.json
was recorded (scripts/make_golden_conv_plan.py) -- return code, all of out8 and the split-K scratch size, row for row."""
import json
import os
import sys

import conv_plan_cases as S
from util import GOLDEN_DIR, ROOT


def test_conv_plan_matches_recorded_table(built_lib):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from make_golden_conv_plan import decode, signatures

    with open(os.path.join(GOLDEN_DIR, "conv_plan_table.json")) as f:
        table = json.load(f)
    want = decode(table)
    rows, digest, reached = S.run_sweep(built_lib)
    assert digest == table["digest"] and len(rows) == table["cases"] == len(want), "the sweep changed: record the table again, on the commit before the change"
    # the table is not thin: every kernel, tile, fused-LayerNorm site, epilogue, ring and split form is in it (and is printed)
    sigs = signatures(want)
    print(f"{len(rows)} cases, {sum(r[0] != 0 for r in want)} rejected; distinct (kernel, tile, ln_fused, launches, form): {sigs}")
    assert [list(s) for s in sigs] == table["signatures"]
    assert sorted(reached) == sorted(S.REQUIRED), f"not reached: {sorted(set(S.REQUIRED) - reached)}"
    assert {tuple(r[1:3]) for r in want if r[0] == 0 and r[7] == 0} == {(256, 32), (256, 64), (256, 256), (128, 128)}
    assert {r[7] for r in want if r[0] == 0} == {0, 2, 3, 4} and any(r[0] != 0 for r in want)
    bad = [(i, w, r) for i, (w, r) in enumerate(zip(want, rows)) if w != r]
    assert not bad, f"{len(bad)} of {len(rows)} answers differ from the table; first (case, recorded, now): {bad[:5]}"
