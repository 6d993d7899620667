"""LPIPS pass timing on one MI355X: N pairs of H x W images (default the benchmark's clip batch, 4 x 17 frames at 256 x 256), per
arithmetic --
  ms per pass of vidtok_amd.lpips.LPIPS (prep + 13 vt_conv_act + 5 vt_lpips_tap + vt_lpips_finish), and the algorithmic TFLOP/s of
  the VGG16 convolutions (2 x 3x3 MACs of both images of every pair, computed from the shapes below);
  the same pass as torch statements (tests/lpips_ref.py: F.conv2d / relu / max_pool2d, head in fp32), timed alternately in the same
  process on the same GPU;
  each tap kernel alone on features of its shape: us and bytes/s (relu_k read once + the pooled write) against 8 TB/s.
Prints a table and one JSON line per arithmetic.  `python scripts/lpips_bench.py [--pairs 68] [--size 256] [--iters 5]`"""
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
from vidtok_amd.lpips import CHNS, LPIPS, TAP_AFTER, VGG_CONVS, VGG_POOLS  # noqa: E402

HBM_BPS = 8e12


def conv_flops(H, W):
    """2 * MACs of the 13 convolutions of ONE image (the first layer at its 3 real input channels)"""
    f, h, w = 0, H, W
    for i in range(30):
        if i in VGG_CONVS:
            cin, cout = VGG_CONVS[i]
            f += 2 * h * w * 9 * cin * cout
        elif i in VGG_POOLS:
            h, w = h // 2, w // 2
    return f


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=68)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--dtypes", default="bf16,fp16,fp32")
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
    y = (x.cpu() + 0.2 * torch.randn(N, 3, S, S, generator=g)).clamp(-1, 1).to(dev)
    gflop = 2 * conv_flops(S, S) / 1e9                    # both images of a pair
    print(f"LPIPS pass: {N} pairs of {S}x{S}, {gflop:.1f} GFLOP per pair (VGG16 3x3 convolutions of both images), "
          f"{gflop * N / 1e3:.2f} TFLOP per pass")
    names = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
    for nm in a.dtypes.split(","):
        dt = names[nm]
        m.set_compute_dtype(dt)
        ours = lambda: m.values(x, y)                                     # noqa: E731
        theirs = lambda: lpips_ref.lpips(sd, x, y, dtype=dt)              # noqa: E731
        with torch.no_grad():
            ours(); ours()
            if not a.no_torch:
                theirs(); theirs()
            t_ours, t_torch = [], []
            for _ in range(3):                                            # alternating rounds
                t_ours.append(timed(ours, a.iters))
                if not a.no_torch:
                    t_torch.append(timed(theirs, a.iters))
        ms = min(t_ours)
        ms_t = min(t_torch) if t_torch else float("nan")
        # the tap kernels alone, on features of their shapes
        taps = []
        work = torch.zeros(ops.lpips_work_bytes(N, S, S) // 4, dtype=torch.float32, device=dev)
        h, w = S, S
        lw = [torch.rand(c, device=dev) for c in CHNS]
        for k, c in enumerate(CHNS):
            feat = F.relu(torch.randn(2 * N, h, w, c, device=dev)).to(dt)
            pool = k < 4
            us = timed(lambda: ops.lpips_tap(feat, lw[k], work, k, pool=pool), 20) * 1e3
            byts = feat.numel() * feat.element_size() * (1.25 if pool else 1.0)
            taps.append(dict(tap=k, shape=[2 * N, h, w, c], us=round(us, 1), tbps=round(byts / us / 1e6, 2)))
            del feat
            h, w = h // 2, w // 2
        rec = dict(metric="lpips_pass", dtype=nm, pairs=N, size=S, ms=round(ms, 3), tflops=round(gflop * N / ms, 1),
                   torch_ms=round(ms_t, 3), speedup_vs_torch=round(ms_t / ms, 2) if t_torch else None,
                   ms_rounds=[round(v, 3) for v in t_ours], torch_ms_rounds=[round(v, 3) for v in t_torch], taps=taps)
        print(f"{nm}: {ms:.2f} ms per pass ({gflop * N / ms:.0f} TFLOP/s algorithmic); torch statements {ms_t:.2f} ms "
              f"(x{ms_t / ms:.2f}); taps: " + ", ".join(f"relu{t['tap'] + 1} {t['us']:.0f} us {t['tbps']:.2f} TB/s "
                                                         f"({100 * t['tbps'] * 1e12 / HBM_BPS:.0f} % of 8 TB/s)" for t in taps))
        print(json.dumps(rec), flush=True)
    m.set_compute_dtype(torch.float32)


if __name__ == "__main__":
    main()
