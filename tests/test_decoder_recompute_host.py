"""Activation recomputation of decode_with_grad (recompute="norms" | "stages"), the part that needs no GPU: the host logic of
vidtok_amd/backward.py run end to end on the torch statements of the operators (tests/torch_ops_ref.py for the forward,
tests/torch_backward_ref.py for the backward).  What is checked is bookkeeping, not numerics: the same operators on the same operands
give the same bits, the tape shrinks, nothing that nobody reads is rebuilt, a parameter changed in place is an error."""
import contextlib
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import backward_sites as S  # noqa: E402
from torch_backward_ref import patched_ops  # noqa: E402
from util import build_model  # noqa: E402

Z = torch.zeros((1, 4, 3, 4, 4))
NEW_MODES = ["norms", "stages"]
SEED = 3


@functools.lru_cache(maxsize=None)
def shared_model(key):
    """one model per config for the whole file: every test leaves it as it found it (fp32, every decoder parameter trainable, seeded values)"""
    return build_model(S.MODELS[key], seed=SEED)[0]


def test_unknown_mode_raises_value_error():
    from vidtok_amd import backward

    model = shared_model("v1_0")
    for call in (model.decode_with_grad, model.decoder.forward_train, functools.partial(backward.forward_train, model.decoder)):
        for mode in ("all", "Norms", None, 1):
            with pytest.raises(ValueError, match="recompute"):
                call(Z, recompute=mode)
    with pytest.raises(ValueError, match="recompute"):
        backward.train_forward(model.decoder, Z, "all")


@pytest.mark.parametrize("what", ["groupnorm", "noncausal", "tiling", "fp16", "bf16x3", "give_pre_end", "tanh_out", "autocast fp16"])
def test_refused_configurations_stay_refused(what):
    """test_decoder_backward_host.py::test_refused_configurations, under the two new modes"""
    name, ov, dtype = "vidtok_kl_causal_488_4chn", None, torch.float32
    if what == "groupnorm":
        ov = {"norm_type": "groupnorm"}
    elif what == "noncausal":
        name = "vidtok_kl_noncausal_488_4chn"
    elif what == "tiling":
        name = "vidtok_v1_1/vidtok_kl_causal_488_4chn_v1_1"
    elif what in ("fp16", "bf16x3"):
        dtype = {"fp16": torch.float16, "bf16x3": "bf16x3"}[what]
    model, _cfg, _sd = build_model(name, dtype=dtype, overrides=ov)
    if what == "tiling":
        model.use_tiling = True
    if what in ("give_pre_end", "tanh_out"):
        setattr(model.decoder, what, True)
    with pytest.raises(ValueError, match="recompute"):           # the mode is looked at before the support checks
        model.decode_with_grad(Z, recompute="everything")
    for mode in NEW_MODES:
        if what == "autocast fp16":
            with torch.autocast("cpu", dtype=torch.float16), pytest.raises(NotImplementedError, match="fp16"):
                model.decode_with_grad(Z, recompute=mode)
        else:
            with pytest.raises(NotImplementedError, match="decode_with_grad"):
                model.decode_with_grad(Z, recompute=mode)


# ---- whole decoder on the torch statements -----------------------------------------------------------------------------------------------
def inputs(model):
    z = torch.randn(Z.shape, generator=torch.Generator().manual_seed(SEED + 1)).requires_grad_(True)
    with torch.no_grad(), patched_ops():
        shape = model.decode(z).shape
    return z, torch.randn(shape, generator=torch.Generator().manual_seed(SEED + 2))


LAST_BACKWARD_CALLS = {}         # operator calls of the latest backward, also of one that raised


def step(model, mode, z=None, cot=None, between=None):
    """one forward + backward on the torch statements: ({name: grad}, x_hat, tape bytes, tape tensors, operator call counts)"""
    from vidtok_amd import backward

    for p in model.decoder.parameters():
        p.grad = None
    if z is None:
        z, cot = inputs(model)
    z.grad = None
    with patched_ops() as calls:
        out = model.decode_with_grad(z, recompute=mode)
        tape = out.grad_fn.tape
        nbytes, ntensors = backward.tape_bytes(tape), len(backward.tape_tensors(tape))
        fwd = dict(calls)
        if between is not None:
            between()
        try:
            (out * cot).sum().backward()
        finally:
            LAST_BACKWARD_CALLS.clear()
            LAST_BACKWARD_CALLS.update({k: v - fwd.get(k, 0) for k, v in calls.items() if v > fwd.get(k, 0)})
    g = {"decoder." + k: p.grad for k, p in model.decoder.named_parameters()}
    g["z"] = z.grad
    bwd = {k: v - fwd.get(k, 0) for k, v in calls.items()}
    return g, out.detach(), nbytes, ntensors, bwd


@functools.lru_cache(maxsize=None)
def whole(key, mode):
    model = shared_model(key)
    return step(model, mode) + (len(model.decoder.train_stage_modules()),)


def assert_same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        assert a[k] is None or torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("mode", NEW_MODES)
@pytest.mark.parametrize("key", ["v1_0", "v1_1"])
def test_same_bits_as_none(key, mode):
    ref, out_ref = whole(key, "none")[:2]
    got, out = whole(key, mode)[:2]
    assert torch.equal(out, out_ref)
    assert all(v is not None and bool(v.abs().sum() > 0) for v in ref.values())
    assert_same_bits(got, ref)


@pytest.mark.parametrize("key", ["v1_0", "v1_1"])
def test_tape_shrinks(key):
    (_g, _o, b_none, _n, bwd_none, n_stages), (_g1, _o1, b_norms, _n1, bwd_norms, _), (_g2, _o2, b_stages, n_tensors, bwd_stages, _) = \
        (whole(key, m) for m in ("none", "norms", "stages"))
    print(f"[tape bytes {key}] none {b_none}, norms {b_norms}, stages {b_stages}")
    assert b_stages < b_norms < b_none
    assert n_tensors == n_stages + 2                 # the latent rows, every stage's input, the tensor in front of norm_out
    # "none" rebuilds nothing; the backward's own launches are the same in every mode
    assert bwd_none.get("layernorm_act", 0) == 0 and bwd_none.get("conv", 0) == 0
    assert bwd_norms["layernorm_act"] > 0 and bwd_norms.get("conv", 0) == 0
    assert bwd_stages["conv"] > 0
    for name in ("conv_wgrad", "conv_dgrad", "layernorm_act_backward"):
        assert bwd_none[name] == bwd_norms[name] == bwd_stages[name], name


def test_tape_bytes_counts_shared_storage_once():
    from vidtok_amd import backward

    a, b = torch.zeros((2, 8)), torch.zeros((3,), dtype=torch.bfloat16)
    empty = [torch.zeros((0,)), torch.zeros((0, 4))]                 # two empty tensors are two tensors (both report address 0)
    tape = backward.Tape(stages=[], saved=[(a, a.view(16), None, torch.Size((1, 2))), [b], empty], cin=None, cout=None, h0=a[0], h=b, hn=None,
                         trim=0, dt=torch.float32, recompute="none", versions=None, arith=None)
    assert backward.tape_bytes(tape) == 2 * 8 * 4 + 3 * 2 and len(backward.tape_tensors(tape)) == 4


@contextlib.contextmanager
def trainable(model, keep):
    """only the decoder parameters `keep(name)` accepts ask for a gradient; all of them again afterwards"""
    try:
        for k, p in model.decoder.named_parameters():
            p.requires_grad_(bool(keep(k)))
        yield
    finally:
        for p in model.decoder.parameters():
            p.requires_grad_(True)


def test_frozen_decoder_rebuilds_no_norm_nobody_reads():
    """every decoder parameter frozen, only z asks: dgrad reads weights only, so "norms" rebuilds no LayerNorm output at all ("stages" has
    to: the pre-norm rows inside a stage come from its forward); the latent's gradient keeps its bits"""
    model = shared_model("v1_1")
    z, cot = inputs(model)
    with trainable(model, lambda k: False):
        ref, out_ref, _b, _n, bwd_ref = step(model, "none", z, cot)
        for mode in NEW_MODES:
            got, out, _b, _n, bwd = step(model, mode, z, cot)
            assert torch.equal(out, out_ref) and ref["z"] is not None
            assert_same_bits(got, ref)
            assert all(v is None for k, v in got.items() if k != "z")
            assert bwd.get("conv_wgrad", 0) == 0 == bwd_ref.get("conv_wgrad", 0)
            if mode == "norms":
                assert bwd.get("layernorm_act", 0) == 0 and bwd.get("conv", 0) == 0
    assert torch.equal(ref["z"], whole("v1_1", "none")[0]["z"])         # and freezing the parameters does not change dz


def test_partly_frozen_and_constant_latent():
    model = shared_model("v1_0")
    frozen = {k for k, p in model.decoder.named_parameters() if k.startswith("up_temporal.") or k.endswith("conv1.weight")}
    z, cot = inputs(model)
    z = z.detach()
    with trainable(model, lambda k: k not in frozen):
        ref = step(model, "none", z, cot)[0]
        for mode in NEW_MODES:
            got = step(model, mode, z, cot)[0]
            assert_same_bits(got, ref)
            assert got["z"] is None and all((got["decoder." + k] is None) == (k in frozen) for k, _p in model.decoder.named_parameters())
    full = whole("v1_0", "none")[0]
    assert all(v is None or torch.equal(v, full[k]) for k, v in ref.items())


@contextlib.contextmanager
def restored(p):
    """the parameter's values as they were, whatever the body did to them"""
    before = p.detach().clone()
    try:
        yield
    finally:
        with torch.no_grad():
            p.copy_(before)


def bump(p):
    def update():
        with torch.no_grad():
            p.add_(1.0)
    return update


def test_parameter_modified_in_place_is_an_error():
    """what optimizer.step() does between forward and backward (an in-place update under no_grad bumps the parameter's version, which is
    also what makes the packed-weight caches repack): the recomputation would run with other weights than the forward.  Noticed before
    anything is launched; a fresh forward + backward is fine, and "none" never minds"""
    model = shared_model("v1_0")
    z, cot = inputs(model)
    params = dict(model.decoder.named_parameters())
    for name in ("mid.block_1.conv1.conv.weight", "up.0.block.0.norm2.norm.bias", "up_temporal.2.upsample.mix_factor"):
        with restored(params[name]):
            for mode in NEW_MODES:
                with pytest.raises(RuntimeError, match=name.replace(".", r"\.")) as e:
                    step(model, mode, z, cot, between=bump(params[name]))
                assert "modified in place" in str(e.value)
                assert LAST_BACKWARD_CALLS == {}, LAST_BACKWARD_CALLS
    last = params["up_temporal.2.upsample.mix_factor"]
    with restored(last):
        step(model, "none", z, cot, between=bump(last))
    for mode in NEW_MODES:
        assert_same_bits(step(model, mode, z, cot)[0], whole("v1_0", "none")[0])


@functools.lru_cache(maxsize=None)
def reference_in(dtype):
    model = shared_model("v1_1")
    try:
        model.set_compute_dtype(dtype)
        return step(model, "none")[0]
    finally:
        model.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("mode", NEW_MODES)
def test_backward_rebuilds_in_the_tapes_arithmetic(mode):
    """the compute dtype (and the weight arithmetic) moves on between forward and backward: the rebuild is the forward's"""
    model = shared_model("v1_1")
    assert not torch.equal(reference_in(torch.bfloat16)["z"], reference_in(torch.float32)["z"])
    try:
        for first, then in ((torch.bfloat16, torch.float32), (torch.float32, "bf16x3")):
            model.set_compute_dtype(first)
            got = step(model, mode, between=lambda: model.set_compute_dtype(then))[0]
            assert model.decoder.compute_dtype == torch.float32 and model.arith == ("fp32" if then == torch.float32 else "bf16x3")
            assert_same_bits(got, reference_in(first))
        assert model.decoder.conv_in.site.pack.arith == "bf16x3"      # and the mode the caller chose is back in force afterwards
    finally:
        model.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("mode", ["none"] + NEW_MODES)
def test_second_backward_fails(mode):
    model = shared_model("v1_0")
    z, cot = inputs(model)
    with patched_ops():
        out = model.decode_with_grad(z, recompute=mode)
        loss = (out * cot).sum()
        loss.backward(retain_graph=True)
        assert out.grad_fn.tape is None
        with pytest.raises(TypeError):
            loss.backward()
