"""Convolution weight-gradient timing on one MI355X: vt_conv_wgrad (ops.conv_wgrad) against the forward convolution of the
same shape (ops.conv), per layer class of the vidtok_kl_causal_488_4chn decoder at B x 17 x 256 x 256, bf16 and fp32.

Both sides do the same algorithmic work, 2 x pixels x Cout x (taps x Cin) FLOPs; TFLOP/s below are that count over the
device-synchronised time of one call (median of --iters after a warm-up).  The wgrad time includes its fixed-order reduce.
Prints a markdown table and one JSON line per row.  `python scripts/wgrad_bench.py [--batch 1] [--iters 10]`"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from vidtok_amd import ops  # noqa: E402
from vidtok_amd.ops import ConvGeom  # noqa: E402

G333 = ConvGeom(kt=3, kh=3, kw=3, pt=2, ph=1, pw=1, ph_hi=1, pw_hi=1)
G311 = ConvGeom(kt=3, pt=2)
G133 = ConvGeom(kh=3, kw=3, ph=1, pw=1, ph_hi=1, pw_hi=1)

# (label, geometry, T, H, W, cin, stored cin, cout): input sizes of the decoder's layer classes at 17 x 256 x 256
CASES = [
    ("conv_in 3x3x3 4->512", G333, 5, 32, 32, 4, 8, 512),
    ("mid 3x3x3 512", G333, 5, 32, 32, 512, 512, 512),
    ("spatial 1x3x3 512 @64", G133, 5, 64, 64, 512, 512, 512),
    ("temporal 3x1x1 512 @64", G311, 9, 64, 64, 512, 512, 512),
    ("spatial 1x3x3 256 @128", G133, 17, 128, 128, 256, 256, 256),
    ("temporal 3x1x1 256 @128", G311, 17, 128, 128, 256, 256, 256),
    ("spatial 1x3x3 128 @256", G133, 17, 256, 256, 128, 128, 128),
    ("temporal 3x1x1 128 @256", G311, 17, 256, 256, 128, 128, 128),
    ("conv_out 3x3x3 128->3", G333, 17, 256, 256, 128, 128, 3),
]


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    dev = "cuda"
    print(f"| layer class (B={args.batch}) | dtype | forward ms | forward TFLOP/s | wgrad ms | wgrad TFLOP/s | wgrad / forward |")
    print("|---|---|---|---|---|---|---|")
    for label, g, T, H, W, cin, ldx, cout in CASES:
        for dt in (torch.bfloat16, torch.float32):
            gen = torch.Generator(device=dev).manual_seed(1)
            x = torch.randn((args.batch, T, H, W, ldx), device=dev, generator=gen).to(dt)
            To, Ho, Wo = g.out_dims(T, H, W)
            dy = torch.randn((args.batch, To, Ho, Wo, ops.pad_channels(cout)), device=dev, generator=gen).to(dt)
            wt = torch.randn((cout, cin, g.kt, g.kh, g.kw), device=dev, generator=gen) * 0.02
            w = ops.pack_conv_weight(wt, dt, cin_stored=ldx)
            b = torch.zeros((cout,), device=dev)
            flops = 2.0 * args.batch * To * Ho * Wo * cout * g.kt * g.kh * g.kw * cin
            t_fwd = timed(lambda: ops.conv(x, w, b, g, cout=cout), args.iters)
            t_wg = timed(lambda: ops.conv_wgrad(x, dy, g, cin=cin, cout=cout), args.iters)
            tf_f, tf_w = flops / t_fwd / 1e9, flops / t_wg / 1e9
            name = {torch.bfloat16: "bf16", torch.float32: "fp32"}[dt]
            print(f"| {label} | {name} | {t_fwd:.3f} | {tf_f:.1f} | {t_wg:.3f} | {tf_w:.1f} | {tf_w / tf_f:.2f} |", flush=True)
            print("JSON " + json.dumps(dict(layer=label, dtype=name, batch=args.batch, fwd_ms=round(t_fwd, 4), wgrad_ms=round(t_wg, 4),
                                            fwd_tflops=round(tf_f, 2), wgrad_tflops=round(tf_w, 2))), file=sys.stderr, flush=True)
            del x, dy, w


if __name__ == "__main__":
    main()
