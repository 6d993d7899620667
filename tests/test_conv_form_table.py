"""vt_conv_launch_form against the recorded table (no GPU): gather form, descriptor extents, skipped time taps, tile order, K steps,
schedule and LDS of the implicit-GEMM launch behind vt_conv, vt_time_upsample3 and vt_conv_act, for every descriptor of the sweep
(tests/conv_form_cases.py), are exactly what the launch code computed when tests/golden/conv_launch_form_table.json was recorded
(scripts/make_golden_conv_plan.py --form) -- return code and all of out16, row for row.  These choices never change a result bit: a layer
class that lost its descriptor gather or its tap skip would only get slower, and this test is what notices."""
import json
import os
import sys

import conv_form_cases as F
from util import GOLDEN_DIR, ROOT


def test_conv_launch_form_matches_recorded_table(built_lib):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from make_golden_conv_plan import decode

    with open(os.path.join(GOLDEN_DIR, "conv_launch_form_table.json")) as f:
        table = json.load(f)
    want = decode(table)
    rows, digest, reached = F.run_sweep(built_lib)
    assert digest == table["digest"] and len(rows) == table["cases"] == len(want), "the sweep changed: record the table again, on the commit before the change"
    # the table is not thin: both gather forms, cache mode on either, taps skipped and not, both tile orders on both tile heights, the
    # 128-tile's epilogues, every schedule, both split forms, the paired and the ReLU launch
    assert sorted(reached) == sorted(F.REQUIRED), f"not reached: {sorted(set(F.REQUIRED) - reached)}"
    igemm = [r[2:] for r in want if r[0] == 0 and r[2 + F.KERNEL] == 0]
    print(f"{len(rows)} cases, {sum(r[0] != 0 for r in want)} rejected, {len(igemm)} implicit-GEMM launches, {len(table['unique'])} distinct answers")
    assert {o[F.BUF] for o in igemm} == {0, 1} and {o[F.TSKIP] for o in igemm} == {0, 1} and {o[F.SCHED] for o in igemm} == {0, 1, 2, 5}
    assert {o[F.KSPLIT] for o in igemm} == {0, 1, 2} and {r[1] for r in want if r[0] == 0} == set(F.CALLS)
    assert all(not any(r[3:]) for r in want if r[0] == 0 and r[2 + F.KERNEL] != 0), "ws2 / narrow / in8 rows report the kernel and zeros"
    bad = [(i, w, r) for i, (w, r) in enumerate(zip(want, rows)) if w != r]
    assert not bad, f"{len(bad)} of {len(rows)} answers differ from the table; first (case, recorded, now): {bad[:5]}"
