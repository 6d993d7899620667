"""Streaming sessions, host side (no GPU): the chunk schedule as a pure function of the push sizes, the per-push emission counts,
the models sessions refuse, and the C entry points' argument checks."""
import ctypes as C
import random

import pytest
import torch

from util import build_model, handle_config


def _tiled_chunks(T, step):
    """AutoencodingEngineV11.build_chunk_start_end, without building a model"""
    from vidtok_amd.engine import AutoencodingEngineV11

    class _Stub:
        t_chunk_enc = t_chunk_dec = step

    return AutoencodingEngineV11.build_chunk_start_end(_Stub(), T)


def _splits(T, rng):
    yield [T]
    yield [1] * T
    yield [1] + [16] * ((T - 1) // 16) + ([(T - 1) % 16] if (T - 1) % 16 else [])
    for _ in range(2):
        out, left = [], T
        while left:
            k = min(left, rng.randint(1, 23))
            out.append(k)
            left -= k
        yield out


def test_schedule_matches_build_chunk_start_end():
    from vidtok_amd.streaming import ChunkSchedule, decode_emission, encode_emission

    rng = random.Random(0)
    for f in (2, 4, 8):
        for c in sorted({f, 2 * f, 16}):
            for T in range(1, 201):
                ref = _tiled_chunks(T, c)
                for split in _splits(T, rng):
                    for look in (0, 1):
                        s = ChunkSchedule(c, look)
                        got, received, counts = [], 0, []
                        for n in split:
                            ready = s.push(n)
                            received += n
                            for a, e, lk in ready:
                                # a chunk runs as soon as it is complete (+ the look-ahead frame), never before
                                assert e + look <= received and lk == bool(look)
                            got += ready
                            counts.append((encode_emission(ready, f), decode_emission(ready, f)))
                        # nothing that could run is still waiting: the next chunk's end (+ look) lies past what arrived
                        nxt = s.start + (1 if s.index == 0 else c)
                        assert nxt + look > received
                        last = s.finish()
                        got += last
                        assert [[a, e] for a, e, _ in got] == ref, (f, c, T, split, look)
                        # tile_decode's look rule: every chunk but the last carries the look-ahead frame (overlap on)
                        assert [lk for _, _, lk in got] == [bool(look) and e + 1 <= T for _, e, _ in got]
                        assert sum(a for a, _ in counts) + encode_emission(last, f) == sum(-(-(e - a) // f) for a, e in ref)
                        assert sum(b for _, b in counts) + decode_emission(last, f) == f * T


def test_emission_counts_per_push():
    """the contract's examples: chunk 0 (the first frame) comes back from the first push; with overlap the decoder lags by one latent"""
    from vidtok_amd.streaming import ChunkSchedule, decode_emission, encode_emission

    s = ChunkSchedule(16)
    assert encode_emission(s.push(1), 4) == 1                     # chunk [0, 1)
    assert encode_emission(s.push(15), 4) == 0                    # 15 of 16 frames of [1, 17)
    assert encode_emission(s.push(1), 4) == 4                     # [1, 17) complete
    assert encode_emission(s.push(22), 4) == 4                    # [17, 33); 6 frames wait
    assert encode_emission(s.finish(), 4) == 2                    # [33, 39): front-padded to 8 frames -> 2 latents
    d = ChunkSchedule(4, lookahead=1)
    assert d.push(1) == []                                        # [0, 1) waits for latent 1
    assert d.push(1) == [(0, 1, True)]
    assert d.push(4) == [(1, 5, True)]                            # needs latent 5, which arrived with this push
    assert d.push(3) == []
    assert decode_emission(d.finish(), 4) == 4 * 4                # [5, 9) without a look-ahead
    n = ChunkSchedule(4)
    assert n.push(1) == [(0, 1, False)] and n.push(4) == [(1, 5, False)]
    assert n.finish() == []                                       # nothing waits
    with pytest.raises(RuntimeError, match="after finish"):
        n.push(1)
    with pytest.raises(RuntimeError, match="twice"):
        n.finish()


@pytest.mark.parametrize("name", ["vidtok_kl_causal_488_4chn", "vidtok_kl_noncausal_488_4chn", "vidtok_fsq_noncausal_488_262144"])
def test_sessions_refuse_v10_and_noncausal(name):
    model, _, _ = build_model(name)
    for opener in (model.open_encode_session, model.open_decode_session, model.open_reconstruct_session):
        with pytest.raises(NotImplementedError, match="v1.1"):
            opener()


def test_session_chunk_must_be_multiple_of_factor():
    model, _, _ = build_model("vidtok_v1_1/vidtok_kl_causal_488_4chn_v1_1")
    for bad in (3, 6, 10):
        with pytest.raises(ValueError, match="multiple"):
            model.open_encode_session(t_chunk_enc=bad)
    assert model.open_encode_session(t_chunk_enc=8).t_chunk_enc == 8
    with pytest.raises(ValueError):
        model.open_decode_session(t_chunk_dec=0)
    model, _, _ = build_model("vidtok_v1_1/vidtok_kl_causal_288_8chn_v1_1")
    with pytest.raises(ValueError):
        model.open_encode_session(t_chunk_enc=5)
    assert model.open_encode_session(t_chunk_enc=6).t_chunk_enc == 6


def test_sessions_take_gpu_tensors_only():
    model, _, _ = build_model("vidtok_v1_1/vidtok_kl_causal_488_4chn_v1_1")
    with pytest.raises(ValueError, match="GPU"):
        model.open_encode_session(8).push(torch.zeros(1, 3, 2, 64, 64))
    with pytest.raises(RuntimeError, match="nothing was pushed"):
        model.open_encode_session(8).finish()


def _handle(built_lib, name):
    from vidtok_amd import lib as L

    import vidtok_amd
    from util import config_path

    cfg = vidtok_amd.load_config(config_path(name))
    prm = cfg["model"]["params"]
    mc = handle_config(L, prm["encoder_config"]["params"], prm["regularizer_config"]["target"], prm["regularizer_config"].get("params", {}),
                       prm["encoder_config"]["target"])
    h = C.c_void_p()
    assert built_lib.vt_create(C.byref(mc), L.VT_F32, C.byref(h)) == 0, built_lib.vt_last_error()
    return h


def test_c_session_entry_points_reject_bad_handles(built_lib):
    from vidtok_amd import lib as L

    s = C.c_void_p()
    assert built_lib.vt_session_create(None, L.VT_SESSION_ENCODE, 1, 64, 64, 16, 0, C.byref(s)) != 0
    assert b"null handle" in built_lib.vt_last_error() and not s.value
    assert built_lib.vt_session_create(None, 0, 1, 64, 64, 16, 0, None) != 0
    for name in ("vidtok_kl_causal_488_4chn", "vidtok_kl_noncausal_488_4chn"):        # v1.0 causal, non-causal
        h = _handle(built_lib, name)
        try:
            for kind in (L.VT_SESSION_ENCODE, L.VT_SESSION_DECODE):
                assert built_lib.vt_session_create(h, kind, 1, 64, 64, 16, 0, C.byref(s)) == -1
                assert b"v1.1" in built_lib.vt_last_error() and not s.value
        finally:
            built_lib.vt_destroy(h)
    h = _handle(built_lib, "vidtok_v1_1/vidtok_kl_causal_488_4chn_v1_1")
    try:
        assert built_lib.vt_session_create(h, L.VT_SESSION_ENCODE, 1, 64, 64, 6, 0, C.byref(s)) == -1
        assert b"multiple of the temporal factor" in built_lib.vt_last_error()
        assert built_lib.vt_session_create(h, 7, 1, 64, 64, 16, 0, C.byref(s)) == -1 and b"kind" in built_lib.vt_last_error()
        assert built_lib.vt_session_create(h, L.VT_SESSION_ENCODE, 1, 60, 64, 16, 0, C.byref(s)) == -1 and b"multiples" in built_lib.vt_last_error()
        # weights not loaded yet: refused before any device memory is taken
        assert built_lib.vt_session_create(h, L.VT_SESSION_ENCODE, 1, 64, 64, 16, 0, C.byref(s)) == -1 and b"not loaded" in built_lib.vt_last_error()
    finally:
        built_lib.vt_destroy(h)
    n = C.c_int32()
    assert built_lib.vt_session_push(None, None, 1, None, 0, C.byref(n), None, 0, None) == -1
    assert built_lib.vt_session_finish(None, None, 0, C.byref(n), None, 0, None) == -1
    assert built_lib.vt_session_workspace_bytes(None) == -1
    assert built_lib.vt_session_destroy(None) == 0
    assert built_lib.vt_copy_segments(None, 0, 0, None) == 0          # nothing to copy: no launch
    assert built_lib.vt_copy_segments(None, 3, 64, None) == -1 and b"table" in built_lib.vt_last_error()
    assert built_lib.vt_copy_segments(None, -1, 64, None) == -1
