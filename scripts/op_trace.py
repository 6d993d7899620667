#!/usr/bin/env python3
"""Operator trace of the Python host mirror, on the CPU: which operator is called, in which order, on which operands.

    python scripts/op_trace.py [--only SUBSTRING] [--dump DIR]

The HIP operators of vidtok_amd.ops are replaced by the torch statements of their contracts (tests/torch_ops_ref.py, tests/torch_backward_ref.py),
each wrapped so that every call writes one line:

    <operator> <parameter>=<value> ... -> <result>

A tensor prints as shape:dtype:hash-of-its-bytes, anything else as its repr (a callable as `callable`).  The arguments are bound to the
operator's signature first, so a default that is spelled out and one that is left out give the same line.  A tensor handed over to be
written (`out`, `ln_out`, `dst`), and a result that is that buffer, print without a hash: until the last launch that fills it, part of it
is memory nobody wrote.  Its content is still held: the next operator that reads it prints its hash.

Seeded models (tests/util.build_model), the smallest clip each config takes.  One SHA-256 per case and one over all lines: two checkouts
whose digests agree launch the same operators on the same operands.  Where they differ, `--dump` writes the lines of every case to a file;
the first differing line names the launch that moved.  Only public names are imported, so the file runs unchanged against older checkouts.
"""
import argparse
import hashlib
import inspect
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch_backward_ref as B  # noqa: E402
import torch_ops_ref as R  # noqa: E402
from util import CONFIG_DIR, build_model  # noqa: E402

import vidtok_amd.ops as ops  # noqa: E402

LINES = []
OUTPUT_PARAMETERS = ("out", "ln_out", "dst")


def tensor_hash(t):
    raw = t.detach().as_subclass(torch.Tensor).contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
    return hashlib.sha1(raw).hexdigest()[:16]


def describe(v, written=()):
    if isinstance(v, torch.Tensor):
        head = f"{tuple(v.shape)}:{str(v.dtype).replace('torch.', '')}"
        return head + (":buffer" if v.untyped_storage().data_ptr() in written else ":" + tensor_hash(v))
    if isinstance(v, (tuple, list)):
        return "[" + ", ".join(describe(e, written) for e in v) + "]"
    if callable(v):
        return "callable"
    return repr(v)


def storages(v):
    if isinstance(v, torch.Tensor):
        return {v.untyped_storage().data_ptr()}
    if isinstance(v, (tuple, list)):
        return set().union(*[storages(e) for e in v]) if v else set()
    return set()


def traced(name, fn):
    sig = inspect.signature(fn)

    def inner(*a, **kw):
        try:
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            args = list(bound.arguments.items())
        except TypeError:            # an argument the torch statement does not know: it will say so itself
            args = [(str(i), v) for i, v in enumerate(a)] + sorted(kw.items())
        written = set()
        for k, v in args:
            if k in OUTPUT_PARAMETERS:
                written |= storages(v)
        line = name + " " + " ".join(f"{k}={describe(v, written)}" for k, v in args)
        result = fn(*a, **kw)
        LINES.append(line + " -> " + describe(result, written))
        return result

    return inner


def copy_segments_statement(pairs, _max_bytes):
    """vt_copy_segments on the host: the pairs themselves stand for the device table"""
    for s, d in pairs:
        d.copy_(s)


def patch():
    for mod, names in ((R, R.ALL), (B, B.ALL)):
        for name in names:
            setattr(ops, name, traced(name, getattr(mod, name)))
    ops.segment_table = lambda pairs, device: (pairs, 0)
    ops.copy_segments = lambda pairs, max_bytes: traced("copy_segments", lambda src: copy_segments_statement(pairs, max_bytes))([s for s, _ in pairs])


class OnGpu(torch.Tensor):
    """a host tensor that answers is_cuda: the sessions take device tensors only; nothing else about it differs"""
    is_cuda = property(lambda self: True)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def config_names():
    out = []
    for base, _dirs, files in os.walk(CONFIG_DIR):
        out += [os.path.relpath(os.path.join(base, f), CONFIG_DIR)[:-len(".yaml")] for f in files if f.endswith(".yaml")]
    return sorted(out)


def smallest_clip(model, frames=None):
    """one full temporal group behind the first frame (causal) or one group (non-causal), two latent pixels each way"""
    enc = model.encoder
    f = enc.time_downsample_factor
    levels = len(getattr(enc, "spatial_ds", range(enc.num_resolutions - 1)))
    t = frames or (1 + f if getattr(enc, "is_causal", False) else f)
    g = torch.Generator().manual_seed(7)
    return torch.rand((1, enc.in_channels, t, 2 << levels, 2 << levels), generator=g) * 2 - 1


def forward_case(name, dtype, **build):
    def run():
        model = build_model(name, seed=3, dtype=dtype, **build)[0]
        torch.manual_seed(1)
        model(smallest_clip(model))
    return run


def tiled_case(name, overlap, frames=17):
    def run():
        model = build_model(name, seed=3)[0]
        model.use_tiling, model.t_chunk_enc, model.t_chunk_dec, model.use_overlap = True, 8, 2, overlap
        torch.manual_seed(1)
        model(smallest_clip(model, frames=frames))      # 17 frames at f = 4: chunks of 1, 8, 8 frames; 5 latent frames in chunks of 1, 2, 2
    return run


def session_case(name):
    def run():
        model = build_model(name, seed=3)[0]
        x = smallest_clip(model, frames=19)
        torch.manual_seed(1)
        enc, zs, t0 = model.open_encode_session(t_chunk_enc=8), [], 0
        for n in (1, 5, 11, 2):
            zs.append(enc.push(x[:, :, t0:t0 + n].as_subclass(OnGpu))[0])
            t0 += n
        zs.append(enc.finish()[0])
        z = torch.cat([t.as_subclass(torch.Tensor) for t in zs], dim=2)
        dec, t0 = model.open_decode_session(t_chunk_dec=2, use_overlap=True), 0
        for n in (2, 1, z.shape[2] - 3):
            dec.push(z[:, :, t0:t0 + n].contiguous().as_subclass(OnGpu))
            t0 += n
        dec.finish()
    return run


def grad_case(name, recompute):
    def run():
        model = build_model(name, seed=3)[0]
        z = torch.randn((1, 4, 3, 4, 4), generator=torch.Generator().manual_seed(4)).requires_grad_(True)
        y = model.decode_with_grad(z, recompute=recompute)
        y.backward(torch.randn(y.shape, generator=torch.Generator().manual_seed(5)))
    return run


def cases():
    out = []
    for name in config_names():
        for dtype in (torch.float32, torch.bfloat16, "bf16x3"):
            out.append((f"forward {name} {str(dtype).replace('torch.', '')}", forward_case(name, dtype)))
    v10, v11 = "vidtok_kl_causal_488_4chn", "vidtok_v1_1/vidtok_kl_causal_488_4chn_v1_1"
    for name in (v10, "vidtok_v1_1/vidtok_kl_causal_488_16chn_v1_1", "vidtok_kl_noncausal_488_4chn"):
        out.append((f"groupnorm {name}", forward_case(name, torch.float32, overrides=dict(norm_type="groupnorm"))))
    out.append(("fsq projections", forward_case("vidtok_fsq_causal_488_32768", torch.float32, overrides=dict(z_channels=8),
                                                reg_overrides=dict(dim=8, levels=[8, 8, 8, 5, 5, 5]))))
    for overlap in (False, True):
        out.append((f"tiled {v11} overlap={overlap}", tiled_case(v11, overlap)))
    # the other temporal factors under overlap (f = 2; f = 8, long enough for a later chunk to carry a look-ahead latent; 16x spatial)
    for name, frames in (("vidtok_v1_1/vidtok_kl_causal_288_8chn_v1_1", 17), ("vidtok_v1_1/vidtok_fsq_causal_888_32768_v1_1", 33),
                         ("vidtok_v1_1/vidtok_kl_causal_41616_16chn_v1_1", 17)):
        out.append((f"tiled {name} overlap=True", tiled_case(name, True, frames)))
    out.append((f"sessions {v11}", session_case(v11)))
    for name in (v10, v11):
        for recompute in ("none", "norms", "stages"):
            out.append((f"decode_with_grad {name} recompute={recompute}", grad_case(name, recompute)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", default="", help="run the cases whose name contains this")
    ap.add_argument("--dump", default=None, help="directory that receives one file of lines per case")
    args = ap.parse_args()
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    patch()
    total = hashlib.sha256()
    for name, run in cases():
        if args.only not in name:
            continue
        del LINES[:]
        run()
        text = "".join(line + "\n" for line in LINES)
        total.update((name + "\n" + text).encode())
        print(f"{hashlib.sha256(text.encode()).hexdigest()[:16]} {len(LINES):5d} {name}", flush=True)
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            with open(os.path.join(args.dump, name.replace("/", "_").replace(" ", "_") + ".txt"), "w") as f:
                f.write(text)
    print(f"sha256 {total.hexdigest()}")


if __name__ == "__main__":
    main()
