"""Activation recomputation of decode_with_grad on the GPU: recompute="norms" and "stages" against "none" on the HIP kernels.

The recomputation launches the forward's kernels on the forward's operands and the kernels are deterministic
(test_gpu_decoder_backward.py::test_two_runs_give_the_same_bits), so every comparison here is torch.equal: there is no tolerance.
Inputs are those of test_gpu_decoder_backward.py::kernel_grads (weights SEED, latent SEED + 1, cotangent SEED + 2)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import backward_sites as S  # noqa: E402
from util import build_model  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 11
NEW_MODES = ["norms", "stages"]
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


@functools.lru_cache(maxsize=None)
def shared_model(key, dtype):
    """one resident model per (config, dtype): every test leaves its parameters and its mode as it found them"""
    return build_model(S.MODELS[key], seed=SEED, device=DEV, dtype=dtype)[0]


def step(model, mode, z_grad=True, autocast=None, between=None, latent=S.LATENT):
    """kernel_grads with a mode: ({name: grad}, x_hat)"""
    for p in model.decoder.parameters():
        p.grad = None
    z = torch.randn(latent, generator=torch.Generator().manual_seed(SEED + 1)).to(DEV).requires_grad_(z_grad)
    if autocast is None:
        out = model.decode_with_grad(z, recompute=mode)
    else:
        with torch.autocast("cuda", dtype=autocast):
            out = model.decode_with_grad(z, recompute=mode)
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(SEED + 2)).to(DEV)
    if between is not None:
        between()
    (out * cot).sum().backward()
    torch.cuda.synchronize()
    g = {"decoder." + k: p.grad for k, p in model.decoder.named_parameters()}
    g["z"] = z.grad
    for p in model.decoder.parameters():
        p.grad = None
    return g, out.detach()


@functools.lru_cache(maxsize=None)
def reference(key, dt):
    """recompute="none": computed once per (config, dtype), shared by the tests, never modified"""
    return step(shared_model(key, DTYPES[dt]), "none")


def assert_same_bits(got, ref):
    assert got.keys() == ref.keys()
    for k in ref:
        assert (got[k] is None) == (ref[k] is None), k
        assert got[k] is None or torch.equal(got[k], ref[k]), k


@pytest.mark.parametrize("mode", NEW_MODES)
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("key", ["v1_0", "v1_1"])
def test_same_bits_as_none(key, dt, mode):
    ref, out_ref = reference(key, dt)
    assert all(v is not None and bool(torch.isfinite(v).all()) and bool((v != 0).any()) for v in ref.values())
    got, out = step(shared_model(key, DTYPES[dt]), mode)
    assert torch.equal(out, out_ref)
    assert_same_bits(got, ref)


def test_backward_after_the_autocast_region():
    """forward inside torch.autocast(bfloat16) on a model whose chosen mode is fp32, backward after the region has ended and after another
    entry point has put the decoder back into fp32: "stages" rebuilds with the bf16 kernels of its forward"""
    ref, out_ref = reference("v1_1", "bf16")
    model = shared_model("v1_1", torch.float32)

    def leave():
        model.decode(torch.zeros(S.LATENT, device=DEV))
        assert model.decoder.compute_dtype == torch.float32 and model.arith == "fp32"

    got, out = step(model, "stages", autocast=torch.bfloat16, between=leave)
    assert torch.equal(out, out_ref)
    assert_same_bits(got, ref)


@pytest.mark.parametrize("mode", NEW_MODES)
def test_frozen_parameters_and_constant_latent(mode):
    model = shared_model("v1_0", torch.bfloat16)
    frozen = {k for k, _p in model.decoder.named_parameters() if k.startswith("up_temporal.")}
    assert frozen
    try:
        for k, p in model.decoder.named_parameters():
            p.requires_grad_(k not in frozen)
        ref, _o = step(model, "none", z_grad=False)
        got, _o = step(model, mode, z_grad=False)
    finally:
        for p in model.decoder.parameters():
            p.requires_grad_(True)
    assert_same_bits(got, ref)
    assert got["z"] is None
    for k, _p in model.decoder.named_parameters():
        assert (got["decoder." + k] is None) == (k in frozen), k
    full, _o = reference("v1_0", "bf16")
    assert all(v is None or torch.equal(v, full[k]) for k, v in got.items())          # and what is left is what the full step gives


@pytest.mark.parametrize("mode", NEW_MODES)
def test_optimizer_step_between_forward_and_backward_is_an_error(mode):
    model = shared_model("v1_0", torch.float32)
    name = "up.1.block.0.conv1.weight"
    p = dict(model.decoder.named_parameters())[name]
    before = p.detach().clone()

    def sgd():
        with torch.no_grad():
            p.add_(torch.ones_like(p), alpha=-1e-3)

    try:
        with pytest.raises(RuntimeError, match=name.replace(".", r"\.")):
            step(model, mode, between=sgd)
    finally:
        with torch.no_grad():
            p.copy_(before)
    ref, out_ref = reference("v1_0", "fp32")
    got, out = step(model, mode)                      # a fresh forward + backward succeeds, on the restored weights with the same bits
    assert torch.equal(out, out_ref)
    assert_same_bits(got, ref)


def test_peak_memory():
    from vidtok_amd import backward

    model = shared_model("v1_0", torch.bfloat16)
    latent = (1, 4, 3, 8, 8)
    step(model, "none", latent=latent)                # packed weights and workspaces of this shape exist before anything is measured
    peak, tape = {}, {}
    for mode in ("none", "norms", "stages"):
        z = torch.randn(latent, generator=torch.Generator().manual_seed(SEED + 1)).to(DEV)
        tape[mode] = backward.tape_bytes(backward.train_forward(model.decoder, z, mode)[1])
        del z
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(model, mode, latent=latent)
        peak[mode] = torch.cuda.max_memory_allocated() - base
    for mode in peak:
        print(f"[recompute memory] latent {latent} bf16 {mode}: peak of forward + backward {peak[mode] / 2 ** 20:.1f} MiB, tape {tape[mode] / 2 ** 20:.1f} MiB")
    assert tape["stages"] < tape["norms"] < tape["none"]
    assert peak["stages"] < peak["none"] and peak["norms"] <= peak["none"]


def frames(v):
    return v.permute(0, 2, 1, 3, 4).reshape(-1, v.shape[1], *v.shape[3:])


def test_chained_with_the_reconstruction_loss():
    """one step of |x - x_hat|.mean() + LPIPS(x, x_hat).mean() at 9 x 32 x 32 (the reconstruction is forward_with_grad's `target`: the
    argument it differentiates); LPIPS weights as in test_gpu_lpips_backward.py"""
    import lpips_backward_ref as R
    from vidtok_amd.lpips import LPIPS

    lp = LPIPS(pretrained=False)
    lp.load_state_dict(R.state_dict(), strict=True)
    lp = lp.to(DEV).eval()
    model = shared_model("v1_0", torch.float32)
    x = (torch.rand(1, 3, 9, 32, 32, generator=torch.Generator().manual_seed(4)) * 2 - 1).to(DEV)
    torch.manual_seed(1)
    z = model.encode(x)

    def run(mode):
        for p in model.decoder.parameters():
            p.grad = None
        zz = z.detach().clone().requires_grad_(True)
        xh = model.decode_with_grad(zz, recompute=mode)
        loss = (x - xh).abs().mean() + lp.forward_with_grad(frames(x), frames(xh)).mean()
        loss.backward()
        torch.cuda.synchronize()
        g = {k: p.grad for k, p in model.decoder.named_parameters()}
        g["z"] = zz.grad
        for p in model.decoder.parameters():
            p.grad = None
        return g, loss.detach()

    ref, loss_ref = run("none")
    got, loss = run("stages")
    assert torch.equal(loss, loss_ref) and all(v is not None and bool((v != 0).any()) for v in ref.values())
    assert_same_bits(got, ref)
