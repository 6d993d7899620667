"""Differentiable decode on one MI355X: decode, training forward, backward, peak memory, and the backward split by kernel class.

    python scripts/decoder_backward_bench.py [--model vidtok_kl_causal_488_4chn] [--frames 17] [--size 256] [--reps 5] [--out profiles/decoder_backward.md]
    python scripts/decoder_backward_bench.py --recompute none,norms,stages --batch 1,4          (the activation-recomputation table alone)

vidtok_kl_causal_488_4chn, B = 1, 17 x 256 x 256, in bf16 and fp32.  Times are medians of `--reps` device-synchronised calls after a
warm-up.  The per-class split comes from event timing: every `ops.*` call of one backward is bracketed by HIP events (the calls are
stream-ordered, so the brackets add up to the whole), classes = dgrad (vt_conv_dgrad: convolution over dy + fold), wgrad
(vt_conv_wgrad + its reduce), LayerNorm backward, attention (GEMMs, softmax backward, transposes), glue (mix, folds, adds, layout).
`--recompute` adds the axis of `decode_with_grad(z, recompute=...)`: per batch size, dtype and mode the training forward, the backward,
the bytes the tape holds between the two (`backward.tape_bytes`) and the peak of forward + backward above the resident model and batch.
Not part of bench.py.
"""
import argparse
import gc
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CLASS_OF = {"conv_dgrad": "dgrad", "conv_wgrad": "wgrad", "layernorm_act_backward": "LayerNorm backward", "gemm_nt": "attention",
            "softmax_rows_backward": "attention", "transpose_batched": "attention", "upsample_mix_backward": "glue", "grad_fold": "glue",
            "grad_add": "glue", "time_lerp2x_backward": "glue", "grad_ncthw_to_ndhwc": "glue", "ndhwc_to_ncthw": "glue"}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def split_backward(model, z, x):
    """ms per kernel class of one backward, and of the dgrad / wgrad calls per layer class (taps, Cin)"""
    from vidtok_amd import ops

    marks, orig = [], {}

    def wrap(name, fn):
        def inner(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **kw)
            e1.record()
            label = ""
            if name in ("conv_dgrad", "conv_wgrad"):
                g = a[2]
                label = f"{g.kt}x{g.kh}x{g.kw} {kw['cin']}->{kw['cout']}"
            marks.append((name, label, e0, e1))
            return r
        return inner

    for name in CLASS_OF:
        orig[name] = getattr(ops, name)
    loss = torch.nn.functional.mse_loss(model.decode_with_grad(z), x)
    torch.cuda.synchronize()
    try:
        for name, fn in orig.items():
            setattr(ops, name, wrap(name, fn))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        for name, fn in orig.items():
            setattr(ops, name, fn)
    per_class, per_layer = {}, {}
    for name, label, e0, e1 in marks:
        ms = e0.elapsed_time(e1)
        per_class[CLASS_OF[name]] = per_class.get(CLASS_OF[name], 0.0) + ms
        if label:
            k = (label, CLASS_OF[name])
            per_layer[k] = per_layer.get(k, 0.0) + ms
    return per_class, per_layer


def recompute_table(args, modes, batches):
    """one row per (batch, dtype, mode); time and memory also as a ratio to recompute="none" of the same run when that is among the modes"""
    from util import build_model
    from vidtok_amd import backward

    lines = [f"## activation recomputation: {args.model}, {args.frames} x {args.size} x {args.size} (scripts/decoder_backward_bench.py --recompute, medians of {args.reps})", "",
             "| B | dtype | recompute | training forward ms | backward ms | tape GiB | peak memory of forward + backward GiB | backward / none | peak / none |",
             "|---|---|---|---|---|---|---|---|---|"]
    for B in batches:
        x = (torch.rand((B, 3, args.frames, args.size, args.size), generator=torch.Generator().manual_seed(0)) * 2 - 1).to("cuda:0")
        for dtype in (torch.bfloat16, torch.float32):
            model, _cfg, _sd = build_model(args.model, seed=7, device="cuda:0", dtype=dtype)
            zg = model.encode(x).clone().requires_grad_(True)
            base_row = None
            for mode in modes:
                def step():
                    for p in model.decoder.parameters():
                        p.grad = None
                    zg.grad = None
                    torch.nn.functional.mse_loss(model.decode_with_grad(zg, recompute=mode), x).backward()

                t_fwd = timed(lambda: model.decode_with_grad(zg, recompute=mode), args.reps)
                t_bwd = timed(step, args.reps) - t_fwd
                tape = backward.tape_bytes(backward.train_forward(model.decoder, zg, mode)[1]) / 2 ** 30
                gc.collect()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                step()
                torch.cuda.synchronize()
                peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
                if mode == "none":
                    base_row = (t_bwd, peak)
                rel = ("-", "-") if base_row is None else (f"{t_bwd / base_row[0]:.3f}", f"{peak / base_row[1]:.3f}")
                lines.append(f"| {B} | {str(dtype).replace('torch.', '')} | {mode} | {t_fwd:.2f} | {t_bwd:.2f} | {tape:.2f} | {peak:.2f} | {rel[0]} | {rel[1]} |")
                print(lines[-1], flush=True)
            del model, zg
            torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="vidtok_kl_causal_488_4chn")
    ap.add_argument("--frames", type=int, default=17)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--recompute", default=None, help="comma-separated modes of decode_with_grad(z, recompute=...): the recomputation table instead of the default report")
    ap.add_argument("--batch", default="1", help="comma-separated batch sizes of the recomputation table")
    args = ap.parse_args()
    from util import build_model

    if args.recompute:
        text = "\n".join(recompute_table(args, args.recompute.split(","), [int(b) for b in args.batch.split(",")])) + "\n"
        print(text)
        if args.out:                     # a section of its own: added to the end of the file, whatever it already holds stays
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(("\n" if os.path.getsize(args.out) else "") + text)
        return

    lines = [f"## {args.model}, B = 1, {args.frames} x {args.size} x {args.size} (scripts/decoder_backward_bench.py, medians of {args.reps})", ""]
    x = (torch.rand((1, 3, args.frames, args.size, args.size), generator=torch.Generator().manual_seed(0)) * 2 - 1).to("cuda:0")
    rows, splits, layers = [], {}, {}
    for dtype in (torch.bfloat16, torch.float32):
        model, _cfg, _sd = build_model(args.model, seed=7, device="cuda:0", dtype=dtype)
        z = model.encode(x)
        t_dec = timed(lambda: model.decode(z), args.reps)
        t_fwd = timed(lambda: model.decode_with_grad(z), args.reps)
        zg = z.clone().requires_grad_(True)

        def step():
            for p in model.decoder.parameters():
                p.grad = None
            zg.grad = None
            torch.nn.functional.mse_loss(model.decode_with_grad(zg), x).backward()

        t_step = timed(step, args.reps)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step()
        torch.cuda.synchronize()
        peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
        rows.append((str(dtype).replace("torch.", ""), t_dec, t_fwd, t_step - t_fwd, peak))
        splits[dtype], layers[dtype] = split_backward(model, zg, x)
        del model
    lines += ["| dtype | decode ms | training forward ms | backward ms | peak memory of forward + backward GiB |", "|---|---|---|---|---|"]
    lines += [f"| {d} | {a:.2f} | {b:.2f} | {c:.2f} | {m:.2f} |" for d, a, b, c, m in rows]
    lines += ["", "Backward by kernel class (event brackets around every op call of one backward, ms and share):", ""]
    classes = sorted({c for s in splits.values() for c in s})
    lines += ["| dtype | " + " | ".join(classes) + " | sum |", "|---|" + "---|" * (len(classes) + 1)]
    for dtype, s in splits.items():
        tot = sum(s.values())
        lines.append(f"| {str(dtype).replace('torch.', '')} | " + " | ".join(f"{s.get(c, 0.0):.2f} ({100 * s.get(c, 0.0) / tot:.0f} %)" for c in classes) + f" | {tot:.2f} |")
    lines += ["", "dgrad and wgrad per layer class (all launches of the class in one backward, ms):", "", "| dtype | layer class | launches' dgrad ms | wgrad ms |", "|---|---|---|---|"]
    for dtype, s in layers.items():
        for label in sorted({k[0] for k in s}):
            lines.append(f"| {str(dtype).replace('torch.', '')} | {label} | {s.get((label, 'dgrad'), 0.0):.3f} | {s.get((label, 'wgrad'), 0.0):.3f} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
