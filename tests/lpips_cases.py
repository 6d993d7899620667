"""LPIPS test cases (TEST INFRASTRUCTURE): seeded inputs and weights, regenerated bit-identically in the build container (where
scripts/make_golden_lpips.py runs the unmodified reference) and on the GPU box (tests/test_gpu_lpips.py)."""
import torch

from util import seeded_state_dict

WEIGHT_SEED = 4321
# form "forward": LPIPS(x, y) on NCHW images in [-1, 1]; form "eval": the eval loop on an NCTHW clip pair (clamp of the
# reconstruction, (v+1)/2, LPIPS on v*2-1), per frame -- its reconstruction leaves [-1, 1] in places, so the clamp matters
CASES = [
    dict(name="p2_32", shape=(2, 3, 32, 32), seed=11, form="forward"),
    dict(name="p3_50x38", shape=(3, 3, 50, 38), seed=12, form="forward"),      # relu5_3: 50 -> 25 -> 12 -> 6 -> 3, 38 -> 19 -> 9 -> 4 -> 2
    dict(name="clip_b2t3_64", shape=(2, 3, 3, 64, 64), seed=13, form="eval"),
]
SCALING = {"scaling_layer.shift": torch.Tensor([-0.030, -0.088, -0.188])[None, :, None, None],
           "scaling_layer.scale": torch.Tensor([0.458, 0.448, 0.450])[None, :, None, None]}


def make_inputs(case):
    g = torch.Generator().manual_seed(case["seed"])
    x = torch.rand(case["shape"], generator=g) * 2 - 1
    noise = torch.randn(case["shape"], generator=g)
    if case["form"] == "eval":
        y = x + 0.35 * noise                      # a "reconstruction" partly outside [-1, 1]
    else:
        y = (x + 0.25 * noise).clamp(-1, 1)
    return x, y


def lpips_state_dict(shapes: dict, seed: int = WEIGHT_SEED) -> dict:
    """seeded weights over the LPIPS key shapes: lin* made non-negative (real LPIPS lin weights are), the ScalingLayer buffers kept
    at the reference's constants"""
    sd = seeded_state_dict(shapes, seed)
    for k in sd:
        if k.startswith("lin"):
            sd[k] = sd[k].abs()
    sd.update({k: v.clone() for k, v in SCALING.items()})
    return sd
