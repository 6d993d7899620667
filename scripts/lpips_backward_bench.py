"""Differentiable LPIPS timing on one MI355X: forward + backward of LPIPS.forward_with_grad over N pairs of H x W images (default the
benchmark's clip batch, 4 x 17 frames at 256 x 256), per arithmetic --
  ms per forward + backward, and the peak bytes allocated above the inputs during it (what the pass keeps + its working set);
  the same pass as torch statements (tests/lpips_ref.py with autograd: F.conv2d / relu / max_pool2d, head in fp32), timed alternately in
  the same process on the same GPU;
  each new kernel alone on tensors of its shapes: us and bytes/s (every operand read once + the result) against 8 TB/s.
Prints a table and one JSON line per arithmetic.  `python scripts/lpips_backward_bench.py [--pairs 68] [--size 256] [--iters 3]`"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lpips_ref  # noqa: E402
from lpips_cases import lpips_state_dict  # noqa: E402

from vidtok_amd import ops  # noqa: E402
from vidtok_amd.lpips import CHNS, LPIPS  # noqa: E402

HBM_BPS = 8e12


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def nbytes(*ts):
    return sum(t.numel() * t.element_size() for t in ts if t is not None)


def kernel_table(N, S, dt, dev):
    rows = []
    h = w = S
    gout = torch.rand(N, device=dev)
    for k, c in enumerate(CHNS):
        feat = F.relu(torch.randn(2 * N, h, w, c, device=dev)).to(dt)
        lw = torch.rand(c, device=dev)
        dpool = torch.randn(N, h // 2, w // 2, c, device=dev) if k < 4 else None          # fp32, as vt_conv_dgrad hands it over
        out = ops.lpips_tap_backward(feat, lw, gout, dpool)
        us = timed(lambda: ops.lpips_tap_backward(feat, lw, gout, dpool), 10) * 1e3
        rows.append(dict(kernel=f"tap_backward relu{k + 1}", shape=[2 * N, h, w, c], us=round(us, 1), tbps=round(nbytes(feat, dpool, out) / us / 1e6, 2)))
        if k == 0:                                                                     # the largest ReLU backward: relu1_1
            dy = torch.randn(N, 1, h, w, c, device=dev)
            y = feat[N:].unsqueeze(1)
            dx = ops.relu_backward(dy, y)
            us = timed(lambda: ops.relu_backward(dy, y), 10) * 1e3
            rows.append(dict(kernel="relu_backward relu1_1", shape=[N, h, w, c], us=round(us, 1), tbps=round(nbytes(dy, y, dx) / us / 1e6, 2)))
            del dy, y, dx
        del feat, dpool, out
        h, w = h // 2, w // 2
    d = torch.randn(N, S, S, 8, device=dev)
    scale = torch.tensor([0.458, 0.448, 0.450], device=dev)
    o = ops.lpips_prep_backward(d, scale)
    us = timed(lambda: ops.lpips_prep_backward(d, scale), 10) * 1e3
    rows.append(dict(kernel="prep_backward", shape=[N, S, S, 8], us=round(us, 1), tbps=round(nbytes(d, o) / us / 1e6, 2)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=68)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    N, S = a.pairs, a.size
    m = LPIPS(pretrained=False)
    m.load_state_dict(lpips_state_dict({k: v.shape for k, v in m.state_dict().items()}), strict=True)
    m = m.to(dev).eval()
    sd = {k: v.to(dev) for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(N, 3, S, S, generator=g) * 2 - 1).to(dev)
    y = (x.cpu() + 0.2 * torch.randn(N, 3, S, S, generator=g)).clamp(-1, 1).to(dev).requires_grad_(True)
    print(f"LPIPS forward + backward: {N} pairs of {S}x{S}")
    for nm in a.dtypes.split(","):
        dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[nm]
        m.set_compute_dtype(dt)

        def ours():
            y.grad = None
            m.forward_with_grad(x, y).mean().backward()

        def theirs():
            y.grad = None
            lpips_ref.lpips(sd, x, y, dtype=dt).mean().backward()

        ours()
        t_fwd = min(timed(lambda: m.forward(x, y), a.iters) for _ in range(2))
        peak = peak_above(ours)
        t_ours, t_torch, peak_t = [], [], None
        if not a.no_torch:
            theirs()
            peak_t = peak_above(theirs)
        for _ in range(3):                                            # alternating rounds
            t_ours.append(timed(ours, a.iters))
            if not a.no_torch:
                t_torch.append(timed(theirs, a.iters))
        y.grad = None
        ms, ms_t = min(t_ours), (min(t_torch) if t_torch else float("nan"))
        rows = kernel_table(N, S, dt, dev)
        rec = dict(metric="lpips_forward_backward", dtype=nm, pairs=N, size=S, ms=round(ms, 3), forward_only_ms=round(t_fwd, 3),
                   peak_bytes=peak, torch_ms=round(ms_t, 3), torch_peak_bytes=peak_t, speedup_vs_torch=round(ms_t / ms, 2) if t_torch else None,
                   ms_rounds=[round(v, 3) for v in t_ours], torch_ms_rounds=[round(v, 3) for v in t_torch], kernels=rows)
        print(f"{nm}: {ms:.2f} ms forward + backward (forward alone {t_fwd:.2f} ms), peak {peak / 2 ** 30:.2f} GiB; torch statements {ms_t:.2f} ms "
              f"(x{ms_t / ms:.2f}), peak {(peak_t or 0) / 2 ** 30:.2f} GiB")
        for r in rows:
            print(f"  {r['kernel']:<24} {str(r['shape']):<22} {r['us']:>8.1f} us  {r['tbps']:.2f} TB/s ({100 * r['tbps'] * 1e12 / HBM_BPS:.0f} % of 8 TB/s)")
        print(json.dumps(rec), flush=True)
    m.set_compute_dtype(torch.float32)


if __name__ == "__main__":
    main()
