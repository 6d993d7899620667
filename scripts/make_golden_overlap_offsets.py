"""Record the cache offsets of an overlapped tiled decode -> tests/golden/overlap_offsets.json (tests/test_chunk_state.py compares the
decoder's offset table against it; no GPU needed).

    python scripts/make_golden_overlap_offsets.py [--out PATH]

{config: {causal convolution's name under `decoder`: offset}} for the seven v1.1 YAMLs, as AutoencodingEngineV11._overlap_offsets
assigned them by hand for f = 2, 4, 8 (autoencoder_v1_1.py:307-320).  That method exists up to commit 9f15836: the table is recorded
there, once, and the decoder's table computed from its structure has to reproduce it.  A row that differs later is a finding about
the change at hand, never a reason to record again."""
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from util import CONFIG_DIR, GOLDEN_DIR  # noqa: E402


def main(argv):
    import vidtok_amd

    rows = {}
    for path in sorted(glob.glob(os.path.join(CONFIG_DIR, "vidtok_v1_1", "*.yaml"))):
        model = vidtok_amd.load_model_from_config(vidtok_amd.load_config(path), verbose=False)
        model._overlap_offsets()
        rows[os.path.relpath(path, CONFIG_DIR)[:-5]] = {n: m.cache_offset for n, m in model.decoder.named_modules() if hasattr(m, "cache_offset")}
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(GOLDEN_DIR, "overlap_offsets.json")
    with open(out, "w") as f:
        json.dump(rows, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{out}: {len(rows)} configs, {sum(len(r) for r in rows.values())} offsets, {os.path.getsize(out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
