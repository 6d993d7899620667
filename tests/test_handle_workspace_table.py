"""The model handle's dry walks against the recorded table (no GPU): vt_workspace_bytes / vt_tile_workspace_bytes of every shipped YAML,
in every arithmetic, answer exactly the integers tests/golden/handle_workspace_table.json holds (scripts/make_golden_handle_workspace.py
recorded them with the library of the commit before csrc/model.cpp was last restructured).  The arenas' peaks sum up every allocation
of both stage graphs in order -- stage outputs, split-K scratch, cache temporaries, the twins allocated only after a probe said yes --
so a moved, dropped or added allocation changes a row."""
import json
import os
import sys

from util import GOLDEN_DIR, ROOT


def test_handle_workspace_matches_recorded_table(built_lib):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from make_golden_handle_workspace import DTYPES, TILE_CASES, VARIANTS, config_names, run_table

    with open(os.path.join(GOLDEN_DIR, "handle_workspace_table.json")) as f:
        want = json.load(f)
    rows = run_table(built_lib)
    n11 = sum("v1_1" in n for n in config_names())
    assert len(rows) == len(DTYPES) * (2 * (len(config_names()) + len(VARIANTS)) + len(TILE_CASES) * (n11 + len(VARIANTS)))
    assert sorted(rows) == sorted(want), "the set of calls changed: record the table again, on the commit before the change"
    # the table is not thin: the sizes differ with the storage width, the chunk settings, the norm kind and the interpolation mode
    assert all(v > 0 for v in want.values())
    assert all(want[k] != want[k.replace("/VT_BF16/", "/VT_F32/")] for k in want if "/VT_BF16/" in k)
    base = VARIANTS[0][0] + "/VT_BF16/"
    assert len({want[base + f"tile_workspace({','.join(map(str, c))})"] for c in TILE_CASES}) == len(TILE_CASES)
    assert len({want[k] for k in want if k.endswith("/VT_BF16/workspace(1,9,64,64)") and k.startswith(VARIANTS[0][0])}) == 1 + len(VARIANTS)
    bad = {k: (want[k], rows[k]) for k in want if want[k] != rows[k]}
    assert not bad, f"{len(bad)} of {len(rows)} sizes differ from the table; first (call: recorded, now): {list(bad.items())[:5]}"
