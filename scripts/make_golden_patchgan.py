#!/usr/bin/env python
"""Record tests/golden/patchgan.safetensors from the UNMODIFIED reference discriminator (build container only).

For train and eval mode at the shapes of tests/patchgan_ref.SHAPES, with the seeded weights and inputs of that module: the fp64 logits,
dx, every parameter gradient's norm and first 64 values, and the running statistics after the call; the state_dict key list and shapes
go into the file's metadata.  tests/test_patchgan_host.py replays the restatement against it where the reference is absent.
"""
import json
import os
import sys

import torch
from safetensors.torch import save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import patchgan_ref as R  # noqa: E402
from oracle import refload  # noqa: E402


def reference_class():
    refload._install_stubs()
    from vidtok.modules.discriminator import NLayerDiscriminator
    return NLayerDiscriminator


def record(net):
    out = {}
    for si, shape in enumerate(R.SHAPES):
        for train in (True, False):
            r = R.run64(net, R.make_inputs(shape, si), train, seed=si)
            tag = f"s{si}.{'train' if train else 'eval'}."
            out[tag + "logits"], out[tag + "dx"] = r["logits"], r["dx"]
            for k, g in r["grads"].items():
                out[tag + "gnorm." + k] = g.norm().reshape(1)
                out[tag + "ghead." + k] = g.reshape(-1)[:64].clone()
            for k, v in r["stats"].items():
                out[tag + "stat." + k] = v
    return out


def main():
    torch.set_num_threads(8)
    net = R.seeded(cls=reference_class())
    out = {k: v.contiguous() for k, v in record(net).items()}
    meta = {"keys": json.dumps({k: list(v.shape) for k, v in net.state_dict().items()})}
    path = os.path.join(ROOT, "tests", "golden", R.GOLDEN)
    save_file(out, path, metadata=meta)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
