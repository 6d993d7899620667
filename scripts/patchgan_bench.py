"""PatchGAN discriminator timing on one MI355X: NLayerDiscriminator over N frames of S x S (default the benchmark's clip batch, 4 x 17
frames at 256 x 256), per arithmetic --
  the forward; forward + generator-side backward (dx only, parameters frozen); forward + discriminator-side backward (parameter gradients
  only, frames detached); the bytes held between the forward and the backward, and the peak during the pair;
  the same steps of the torch.nn module (tests/patchgan_ref.py; bf16 under torch.autocast), timed alternately in the same process;
  every launch class of our pass on its own (a synchronise around each ops.* call: kernel time + launch overhead), so that a step that
  loses to torch names its launch.
Prints a table and one JSON line per arithmetic.  `python scripts/patchgan_bench.py [--frames 68] [--size 256] [--iters 5]`"""
import argparse
import collections
import json
import os
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import patchgan_ref as R  # noqa: E402

from vidtok_amd import ops  # noqa: E402
from vidtok_amd.discriminator import NLayerDiscriminator  # noqa: E402

OPS = ("ncthw_to_ndhwc", "conv", "batchnorm_stats", "batchnorm_act", "grad_ncthw_to_ndhwc", "conv_wgrad", "conv_dgrad", "batchnorm_act_backward",
       "leaky_relu_backward", "ndhwc_to_ncthw")


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def held_and_peak(fwd):
    """(bytes still allocated after the forward, i.e. kept for the backward; peak above the start during forward + backward)"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y = fwd()
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - base
    y.mean().backward()
    torch.cuda.synchronize()
    return held, torch.cuda.max_memory_allocated() - base


class Breakdown:
    """per-launch-class milliseconds of one pass: every ops.* call of the discriminator between two synchronises"""

    def __enter__(self):
        self.ms, self.real = collections.OrderedDict(), {}
        for name in OPS:
            self.real[name] = fn = getattr(ops, name)

            def wrap(*a, _fn=fn, _name=name, **kw):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = _fn(*a, **kw)
                torch.cuda.synchronize()
                key = _name + (f" cout={kw['cout']}" if "cout" in kw else "")
                self.ms[key] = self.ms.get(key, 0.0) + (time.perf_counter() - t0) * 1e3
                return out

            setattr(ops, name, wrap)
        return self

    def __exit__(self, *exc):
        for name, fn in self.real.items():
            setattr(ops, name, fn)
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=68)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--dtypes", default="bf16,fp32")
    a = ap.parse_args()
    dev = "cuda:0"
    N, S = a.frames, a.size
    ref = R.seeded().to(dev).train()
    d = NLayerDiscriminator()
    d.load_state_dict(ref.state_dict(), strict=True)
    d = d.to(dev).train()
    x = (torch.rand(N, 3, S, S, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
    xg = x.clone().requires_grad_(True)
    print(f"PatchGAN discriminator (train mode): {N} frames of {S}x{S}")
    for nm in a.dtypes.split(","):
        dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[nm]
        d.set_compute_dtype(dt)

        def cast():
            return torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16)

        def freeze(mod, frozen):
            for p in mod.parameters():
                p.requires_grad_(not frozen)
                p.grad = None

        def t_fwd():
            with torch.no_grad(), cast():
                return ref(x)

        def step(mod, call, gen):
            """forward + backward of the generator side (gen: dx only) or the discriminator side (parameter gradients only)"""
            xg.grad = None
            for p in mod.parameters():
                p.grad = None
            call(xg if gen else x).mean().backward()

        def t_call(v):
            with cast():
                return ref(v)

        rec = dict(metric="patchgan", dtype=nm, frames=N, size=S)
        sides = {}
        for side, gen in (("generator", True), ("discriminator", False)):
            freeze(d, gen), freeze(ref, gen)
            ours = lambda: step(d, d.forward_with_grad, gen)        # noqa: E731
            theirs = lambda: step(ref, t_call, gen)                 # noqa: E731
            ours(), theirs()
            held, peak = held_and_peak(lambda: d.forward_with_grad(xg if gen else x))
            held_t, peak_t = held_and_peak(lambda: t_call(xg if gen else x))
            to, tt = [], []
            for _ in range(3):                                      # alternating rounds
                to.append(timed(ours, a.iters))
                tt.append(timed(theirs, a.iters))
            with Breakdown() as b:
                ours()
            sides[side] = dict(ms=round(min(to), 3), torch_ms=round(min(tt), 3), ms_rounds=[round(v, 3) for v in to], torch_ms_rounds=[round(v, 3) for v in tt],
                               held_bytes=held, peak_bytes=peak, torch_held_bytes=held_t, torch_peak_bytes=peak_t,
                               launches={k: round(v, 3) for k, v in b.ms.items()})
        freeze(d, False), freeze(ref, False)
        d(x), t_fwd()
        fo, ft = [], []
        for _ in range(3):
            fo.append(timed(lambda: d(x), a.iters))
            ft.append(timed(t_fwd, a.iters))
        rec.update(forward_ms=round(min(fo), 3), torch_forward_ms=round(min(ft), 3), **sides)
        print(f"{nm}: forward {min(fo):.2f} ms (torch {min(ft):.2f})")
        for side, s in sides.items():
            print(f"  {side} step, forward + backward: {s['ms']:.2f} ms (torch {s['torch_ms']:.2f}); backward alone {s['ms'] - min(fo):.2f} ms (torch "
                  f"{s['torch_ms'] - min(ft):.2f}); held for the backward {s['held_bytes'] / 2 ** 20:.0f} MiB (torch {s['torch_held_bytes'] / 2 ** 20:.0f}), "
                  f"peak {s['peak_bytes'] / 2 ** 20:.0f} MiB (torch {s['torch_peak_bytes'] / 2 ** 20:.0f})")
            for k, v in s["launches"].items():
                print(f"      {k:<34} {v:8.3f} ms")
        print(json.dumps(rec), flush=True)
    d.set_compute_dtype(torch.float32)


if __name__ == "__main__":
    main()
