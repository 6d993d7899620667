"""CPU tests of the host's chunk state (vidtok_amd/chunks.py): one ChunkState per encoder / decoder over the slots of its caching
modules, written by the engine and the sessions only.  The HIP operators are replaced by the torch statements of their contracts
(tests/torch_ops_ref.py)."""
import json
import os

import pytest
import torch

import torch_ops_ref
from util import GOLDEN_DIR, build_model, config_path

V11 = "vidtok_v1_1/vidtok_kl_causal_488_4chn_v1_1"


@pytest.fixture()
def emulated_ops(monkeypatch):
    torch_ops_ref.patch_ops(monkeypatch)


def tiled_model(**overrides):
    model = build_model(V11, seed=3, overrides=overrides or None)[0]
    model.use_tiling, model.t_chunk_dec = True, 2
    return model


def latent():
    return torch.randn((1, 4, 5, 4, 4), generator=torch.Generator().manual_seed(4))


@pytest.mark.parametrize("order", [(True, False), (False, True)], ids=["overlap_then_plain", "plain_then_overlap"])
def test_a_pass_does_not_inherit_the_previous_overlap(order, emulated_ops):
    """Two tiled decodes on one model, with and without the look-ahead latent, in either order: the second gives the bits of a fresh
    model's.  Before the chunk state had one owner this failed for overlap -> plain (up to 1.41 in absolute value): tile_decode wrote
    the cache offsets only when use_overlap was set and nothing took them back, so every causal convolution still skipped 1, 2 or 4
    frames."""
    z = latent()
    model = tiled_model()
    for overlap in order:
        model.use_overlap = overlap
        got = model.decode(z)
    fresh = tiled_model()
    fresh.use_overlap = order[1]
    assert torch.equal(got, fresh.decode(z))


def test_overlap_offsets_match_the_recorded_table():
    """the decoder's offset table, computed from its structure, against what the engine assigned by hand for f = 2, 4, 8
    (tests/golden/overlap_offsets.json, scripts/make_golden_overlap_offsets.py); without overlap every offset is zero"""
    import vidtok_amd
    from vidtok_amd.modules import CausalConv1d, CausalConv3d

    with open(os.path.join(GOLDEN_DIR, "overlap_offsets.json")) as f:
        table = json.load(f)
    assert len(table) == 7
    for name, want in table.items():
        dec = vidtok_amd.load_model_from_config(vidtok_amd.load_config(config_path(name)), verbose=False).decoder
        convs = {n: m for n, m in dec.named_modules() if isinstance(m, (CausalConv1d, CausalConv3d))}
        dec.chunks.set_overlap(True)
        assert {n: m.slot.offset for n, m in convs.items()} == want, name
        dec.chunks.set_overlap(False)
        assert not any(s.offset for s in dec.chunks.slots), name


def test_overlap_is_refused_for_other_temporal_factors(emulated_ops):
    model = tiled_model(time_downsample_factor=16)
    model.use_overlap = True
    with pytest.raises(AssertionError, match="2x, 4x or 8x"):
        model.decode(latent())
    assert model.decoder.chunks.overlap_table is None and not any(s.offset for s in model.decoder.chunks.slots)
    model.decoder.chunks.set_overlap(False)           # only the overlapped pass is refused


class OnGpu(torch.Tensor):
    """a host tensor that answers is_cuda: the sessions take device tensors only; nothing else about it differs"""
    is_cuda = property(lambda self: True)


def test_failed_push_leaves_both_states_as_before(emulated_ops, monkeypatch):
    """a session push whose chunk raises puts both halves' chunk states back: flags, offsets and the very cache tensors"""
    import vidtok_amd.ops as ops

    def copy_pairs(pairs, _max_bytes):
        for s, d in pairs:
            d.copy_(s)

    monkeypatch.setattr(ops, "segment_table", lambda pairs, device: (pairs, 0))
    monkeypatch.setattr(ops, "copy_segments", copy_pairs)
    model = tiled_model()
    z = latent()
    model.decode(z)                                   # a plain pass leaves caches bound and first = False: a state worth comparing

    def states():
        return [st.snapshot() for st in model._chunk_states()]

    def same(a, b):
        return all(sa[:3] == sb[:3] and len(sa[3]) == len(sb[3]) and all(ca is cb and oa == ob for (ca, oa), (cb, ob) in zip(sa[3], sb[3]))
                   for sa, sb in zip(a, b))

    before = states()
    assert any(c is not None for c, _ in before[1][3]) and before[1][:3] == (False, True, False)
    dec = model.open_decode_session(t_chunk_dec=2, use_overlap=True)
    dec.push(z[:, :, :2].contiguous().as_subclass(OnGpu))            # chunk 0 runs: offsets, flags and caches change inside the push
    assert same(states(), before)

    def broken(*a, **kw):
        raise RuntimeError("operator failed")

    monkeypatch.setattr(ops, "layernorm_act", broken)
    with pytest.raises(RuntimeError, match="operator failed"):
        dec.push(z[:, :, 2:].contiguous().as_subclass(OnGpu))
    assert same(states(), before)
