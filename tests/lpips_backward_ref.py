"""References of the LPIPS backward tests (TEST INFRASTRUCTURE, CPU only): the seeded weights, the fp64 autograd gradient of
tests/lpips_ref.py with respect to the reconstruction and its bf16 counterpart, each computed once per case and shared by
tests/test_lpips_backward_host.py and tests/test_gpu_lpips_backward.py (callers must not modify what they get)."""
import functools

import torch
import torch.nn.functional as F

import lpips_ref
from lpips_cases import CASES, lpips_state_dict, make_inputs

GRAD_CASES = CASES[:2]                     # p2_32, p3_50x38 (odd pooling: 50 -> 25 -> 12 -> 6 -> 3, 38 -> 19 -> 9 -> 4 -> 2)


def pair_weights(n):
    """fixed non-uniform cotangent of the N LPIPS values"""
    return torch.linspace(0.5, 1.5, n) * (1 - 2 * (torch.arange(n) % 2))          # 0.5, -1.0, 1.5, ...


@functools.lru_cache(maxsize=1)
def state_dict():
    from vidtok_amd.lpips import LPIPS

    m = LPIPS(pretrained=False)
    return lpips_state_dict({k: v.shape for k, v in m.state_dict().items()})


def _grad(case, dtype):
    x, y = make_inputs(case)
    sd = state_dict()
    if dtype == torch.float64:
        sd = {k: v.double() for k, v in sd.items()}
        x, y = x.double(), y.double()
    y = y.clone().requires_grad_(True)
    val = lpips_ref.lpips(sd, x, y, dtype=dtype)
    (val.double() * pair_weights(val.numel()).double()).sum().backward()
    return y.grad.double()


@functools.lru_cache(maxsize=None)
def ref_grad(name):
    """fp64 CPU autograd gradient of sum(wts * lpips_ref.lpips(x, y)) with respect to y"""
    return _grad(next(c for c in CASES if c["name"] == name), torch.float64)


@functools.lru_cache(maxsize=None)
def bf16_grad(name):
    """the same gradient with lpips_ref's convolutions in bf16 on the CPU (torch autograd): the baseline of the bf16 gate"""
    return _grad(next(c for c in CASES if c["name"] == name), torch.bfloat16)


def zero_pixels_per_tap(case):
    """number of all-zero pixels of the reconstruction's features at each of the five taps (fp64)"""
    x, y = make_inputs(case)
    sd = {k: v.double() for k, v in state_dict().items()}
    h = (y.double() - sd["scaling_layer.shift"]) / sd["scaling_layer.scale"]
    with torch.no_grad():
        return [int((t.abs().sum(1) == 0).sum()) for t in lpips_ref.vgg_taps(sd, h, torch.float64)]


def ref_tap_backward(feat, lin_w, gout, dpool):
    """fp64 autograd of the head of one tap + max_pool2d + the ReLU mask on the features the kernel reads: feat [2N, H, W, C]
    (already rounded to the storage type), dpool [N, H/2, W/2, C] or None -> [N, H, W, C].  The norm's own gradient is taken as 0
    at an all-zero pixel (where(s > 0, ..., 0)): torch's sqrt backward would give NaN there."""
    f = feat.double().permute(0, 3, 1, 2)
    N = f.shape[0] // 2
    z = f[N:].clone().requires_grad_(True)                     # stands for the pre-activation: relu(z) == f1, relu'(z) = [f1 > 0]
    f0, f1 = f[:N], F.relu(z)

    def unit(t):
        ss = (t ** 2).sum(1, keepdim=True)
        s = torch.where(ss > 0, torch.where(ss > 0, ss, torch.ones_like(ss)).sqrt(), torch.zeros_like(ss))
        return t / (s + 1e-10)

    d = (unit(f0) - unit(f1)) ** 2
    val = (d * lin_w.double()[None, :, None, None]).sum(1).mean([1, 2])
    loss = (val * gout.double()).sum()
    if dpool is not None:
        loss = loss + (F.max_pool2d(f1, 2, 2) * dpool.double().permute(0, 3, 1, 2)).sum()
    loss.backward()
    return z.grad.permute(0, 2, 3, 1)
