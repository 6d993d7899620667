"""Build-container helper: LPIPS of the UNMODIFIED reference (vidtok/modules/lpips.py, loaded by tests/lpips_refload.py without
torchvision or network) on the seeded cases of tests/lpips_cases.py -> tests/golden/lpips.safetensors: per case the per-pair (or
per-frame, eval-loop form) values `<case>/lpips` and the five per-tap spatial means `<case>/taps` [5, N].  Inputs and weights are
regenerated from the seeds; only the reference's outputs are stored.  Re-run: `python scripts/make_golden_lpips.py`."""
import os
import sys

import torch
from safetensors.torch import save_file

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from lpips_cases import CASES, lpips_state_dict, make_inputs  # noqa: E402
from lpips_refload import reference_lpips, reference_taps  # noqa: E402
from util import GOLDEN_DIR  # noqa: E402


def main():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    ref = reference_lpips(use_dropout=True)
    sd = lpips_state_dict({k: v.shape for k, v in ref.state_dict().items()})
    ref.load_state_dict(sd, strict=True)
    out = {}
    with torch.no_grad():
        for case in CASES:
            x, y = make_inputs(case)
            if case["form"] == "eval":            # scripts/inference_evaluate.py:175-186, per frame
                o = y.clamp(-1, 1)
                inp, o = (x + 1) / 2, (o + 1) / 2
                B, C, T, H, W = x.shape
                inp = inp.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W)
                o = o.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W)
                x, y = inp * 2 - 1, o * 2 - 1
            out[case["name"] + "/lpips"] = ref(x, y).reshape(-1).contiguous()
            out[case["name"] + "/taps"] = reference_taps(ref, x, y).contiguous()
            print(case["name"], out[case["name"] + "/lpips"].tolist())
    save_file(out, os.path.join(GOLDEN_DIR, "lpips.safetensors"))


if __name__ == "__main__":
    main()
