"""The pointwise and backward entry points against the recorded refusal table (no GPU): every call of
tests/golden/entry_refusal_table.json (scripts/make_golden_entry_refusals.py recorded it with the library of the commit before their
launch code moved onto csrc/launch.h) is refused with the recorded status and the recorded vt_last_error text, byte for byte.  Every
row is refused before anything is launched, and only rows of the table are called, so nothing here reaches a launch."""
import json
import os
import sys
from collections import Counter

from util import GOLDEN_DIR, ROOT


def test_entry_refusals_match_recorded_table(built_lib):
    from vidtok_amd import lib as L

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from make_golden_entry_refusals import CALLS, VT_ERR_ARG, call, dtype_entries, key

    with open(os.path.join(GOLDEN_DIR, "entry_refusal_table.json")) as f:
        want = json.load(f)
    calls = {key(name, args): (name, args) for name, args in CALLS}
    assert len(calls) == len(CALLS)
    assert sorted(calls) == sorted(want), "the set of calls changed: record the table again, on the commit before the change"
    assert all(v[0] == VT_ERR_ARG and v[1] for v in want.values())
    # the table is not thin: every entry point that takes a storage type has its unknown-dtype row and at least one more
    per_name = Counter(name for name, _ in CALLS)
    entries = dtype_entries()
    assert len(entries) >= 30 and all(n in L.SIGNATURES for n in entries)
    thin = [n for n in entries if per_name[n] < 2 or not any("99" in k for k in calls if k.startswith((n + "(", n + "{")))]
    assert not thin, f"entry points with a dtype argument and fewer than two rows (or no dtype-99 row): {thin}"
    bad = {}
    for k in sorted(want):                       # only rows of the table are ever called
        got = list(call(built_lib, *calls[k]))
        if got[0] != want[k][0] or got[1].encode() != want[k][1].encode():
            bad[k] = (want[k], got)
    assert not bad, f"{len(bad)} of {len(want)} refusals differ from the table; first (call: recorded, now): {list(bad.items())[:5]}"
