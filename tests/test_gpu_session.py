"""Streaming sessions of the v1.1 models on the GPU: every output bit-equal to the tiled whole-clip path (torch.equal, no
tolerance), however the clip is split into pushes; sessions independent of each other and of plain model calls; device memory
bounded by the chunk; the C sessions byte-equal to vt_tile_encode / vt_tile_decode; vt_copy_segments against torch copies."""
import ctypes as C
import os
import random
import shutil
import subprocess

import pytest
import torch

from util import ROOT, build_model, handle_config

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
X3 = "bf16x3"
F16 = torch.float16
V11 = "vidtok_v1_1/"


def _model(name, dtype=torch.bfloat16, c=16, overlap=True, sample=False, seed=11):
    model, cfg, sd = build_model(V11 + name, seed=seed, device=DEV, dtype=dtype)
    if hasattr(model.regularization, "sample"):
        model.regularization.sample = sample
    f = model.encoder.time_downsample_factor
    model.use_tiling, model.t_chunk_enc, model.t_chunk_dec, model.use_overlap = True, c, c // f, overlap
    return model, cfg, sd


def _clip(T, seed=0, B=1, hw=64):
    return (torch.rand((B, 3, T, hw, hw), generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(DEV)


def _splits(T, c=16, seed=0):
    rng = random.Random(seed)
    ragged, left = [], T
    while left:
        k = min(left, rng.randint(1, 2 * c + 3))
        ragged.append(k)
        left -= k
    steady = [1] + [c] * ((T - 1) // c) + ([(T - 1) % c] if (T - 1) % c else [])
    return {"whole": [T], "ones": [1] * T, "steady": steady, "ragged": ragged}


def _encode(session, x, split):
    zs, idx, t = [], [], 0
    for n in split:
        z, log = session.push(x[:, :, t:t + n])
        t += n
        zs.append(z)
        idx.append(log.get("indices"))
    z, log = session.finish()
    zs.append(z)
    idx.append(log.get("indices"))
    return torch.cat(zs, 2), (torch.cat(idx, 1) if idx[0] is not None else None)


def _decode(session, z, split):
    outs, t = [], 0
    for n in split:
        outs.append(session.push(z[:, :, t:t + n] if z.dim() == 5 else z[:, t:t + n]))
        t += n
    outs.append(session.finish())
    return torch.cat(outs, 2)


ENC_CONFIGS = ["vidtok_kl_causal_488_4chn_v1_1", "vidtok_fsq_causal_488_32768_v1_1", "vidtok_kl_causal_288_8chn_v1_1",
               "vidtok_fsq_causal_888_32768_v1_1", "vidtok_kl_causal_41616_16chn_v1_1"]


@pytest.mark.parametrize("name", ENC_CONFIGS)
def test_encode_session_equals_tile_encode(name):
    """T = 39, c = 16: chunks [0,1) [1,17) [17,33) [33,39) -- the last one partial; every push pattern gives tile_encode's bits"""
    model, _, _ = _model(name)
    x = _clip(39, seed=1)
    z_ref, log_ref = model.encode(x, return_reg_log=True)
    for kind, split in _splits(39).items():
        z, idx = _encode(model.open_encode_session(16), x, split)
        assert z.shape == z_ref.shape and torch.equal(z, z_ref), kind
        if "indices" in log_ref:
            assert torch.equal(idx, log_ref["indices"]), kind


@pytest.mark.parametrize("dtype", [F16, torch.float32, X3], ids=["fp16", "fp32", "bf16x3"])
def test_encode_session_other_arithmetics(dtype):
    model, _, _ = _model("vidtok_kl_causal_488_4chn_v1_1", dtype=dtype)
    x = _clip(39, seed=2)
    z_ref = model.encode(x)
    for kind in ("ones", "ragged"):
        z, _ = _encode(model.open_encode_session(16), x, _splits(39, seed=3)[kind])
        assert torch.equal(z, z_ref), (dtype, kind)


def test_session_follows_autocast_and_refuses_a_change():
    model, _, _ = _model("vidtok_kl_causal_488_4chn_v1_1", dtype=torch.float32)
    x = _clip(21, seed=4)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        z_ref = model.encode(x)
        s = model.open_encode_session(16)
        z, _ = _encode(s, x, [1, 7, 13])
    assert torch.equal(z, z_ref)
    s = model.open_encode_session(16)
    s.push(x[:, :, :5])
    with torch.autocast("cuda", dtype=torch.float16):
        with pytest.raises(RuntimeError, match="arithmetic changed"):
            s.push(x[:, :, 5:9])
    with pytest.raises(ValueError, match="differ"):
        s.push(x[:, :, 5:9, :32])
    s.finish()
    with pytest.raises(RuntimeError, match="finished"):
        s.push(x[:, :, 9:10])


@pytest.mark.parametrize("name,overlap,from_indices", [
    ("vidtok_kl_causal_488_4chn_v1_1", True, False), ("vidtok_kl_causal_488_4chn_v1_1", False, False),
    ("vidtok_fsq_causal_488_32768_v1_1", True, True), ("vidtok_fsq_causal_488_32768_v1_1", False, True),
    ("vidtok_kl_causal_288_8chn_v1_1", True, False)], ids=["kl_overlap", "kl_no_overlap", "fsq_idx_overlap", "fsq_idx_no_overlap", "kl288_overlap"])
def test_decode_session_equals_tile_decode(name, overlap, from_indices):
    model, _, _ = _model(name, overlap=overlap)
    x = _clip(45, seed=5)
    z, log = model.encode(x, return_reg_log=True)
    src = log["indices"] if from_indices else z
    ref = model.decode(src, decode_from_indices=from_indices)
    Tz = z.shape[2]
    c = model.t_chunk_dec
    for kind, split in _splits(Tz, c=c, seed=6).items():
        got = _decode(model.open_decode_session(use_overlap=overlap, from_indices=from_indices), src, split)
        assert got.shape == ref.shape and torch.equal(got, ref), kind


@pytest.mark.parametrize("overlap", [True, False])
def test_reconstruct_session_equals_tiled_forward(overlap):
    model, _, _ = _model("vidtok_fsq_causal_488_32768_v1_1", overlap=overlap)
    for T, split in ((39, [1, 16, 16, 6]), (33, [5, 9, 19]), (17, [17])):
        x = _clip(T, seed=T)
        _, dec_ref, _ = model(x)
        s = model.open_reconstruct_session()
        outs = [s.push(x[:, :, a:a + n]) for a, n in zip([sum(split[:i]) for i in range(len(split))], split)]
        tail, drop = s.finish()
        full = torch.cat(outs + [tail], 2)
        assert drop == full.shape[2] - T and drop >= 0
        assert torch.equal(full[:, :, drop:], dec_ref), (T, split)


def test_kl_host_noise_matches_seeded_tile_encode():
    model, _, _ = _model("vidtok_kl_causal_488_4chn_v1_1", sample=True)
    x = _clip(41, seed=7)
    torch.manual_seed(123)
    z_ref, log_ref = model.encode(x, return_reg_log=True)
    torch.manual_seed(123)
    s = model.open_encode_session(16)
    z, _ = _encode(s, x, [3, 20, 18])
    assert torch.equal(z, z_ref)
    assert len(s.chunk_losses) == 4
    assert torch.equal(s.reg_log()["kl_loss"], log_ref["kl_loss"])


def test_graphs_on_and_off_same_bits():
    model, _, _ = _model("vidtok_kl_causal_488_4chn_v1_1", c=8)
    x = _clip(37, seed=8)
    z_ref = model.encode(x)
    d_ref = model.decode(z_ref)
    model.enable_graphs()
    for rnd in range(3):             # eager (first sight of a kind), capture, replay
        z, _ = _encode(model.open_encode_session(8), x, [1, 8, 8, 5, 15])
        d = _decode(model.open_decode_session(), z, [2, 3, 5])
        assert torch.equal(z, z_ref) and torch.equal(d, d_ref), rnd
    assert any(isinstance(e, tuple) for e in model._genc.entries.values())          # chunks did replay from graphs


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
def test_two_sessions_interleaved_and_plain_calls_between(graphs):
    model, _, _ = _model("vidtok_fsq_causal_488_32768_v1_1", c=8)
    if graphs:
        model.enable_graphs()
    xa, xb, xc = _clip(29, seed=9), _clip(29, seed=10), _clip(13, seed=11)
    alone = [model.encode(x, return_reg_log=True) for x in (xa, xb)]
    plain = model(xc)
    sa, sb = model.open_encode_session(8), model.open_encode_session(8)
    za, zb = [], []
    for a in range(0, 29, 4):
        za.append(sa.push(xa[:, :, a:a + 4])[0])
        mid = model(xc)                                   # a plain forward between the pushes: its own bits ...
        assert torch.equal(mid[1], plain[1]) and torch.equal(mid[0], plain[0])
        zb.append(sb.push(xb[:, :, a:a + 4])[0])
    za.append(sa.finish()[0])
    zb.append(sb.finish()[0])
    # ... and the sessions' bits
    assert torch.equal(torch.cat(za, 2), alone[0][0]) and torch.equal(torch.cat(zb, 2), alone[1][0])
    assert sa.switches >= 4


def test_session_memory_bounded_by_chunk():
    model, _, _ = _model("vidtok_kl_causal_488_4chn_v1_1")
    xs = {T: (torch.rand((1, 3, T, 64, 64), generator=torch.Generator().manual_seed(T)) * 2 - 1) for T in (33, 161)}

    def session_peak(T):
        s = model.open_encode_session(16)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        for a in range(0, T, 16):
            s.push(xs[T][:, :, a:a + 16].to(DEV))[0].cpu()
        s.finish()[0].cpu()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    def tiled_peak(T):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        model.encode(xs[T].to(DEV)).cpu()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    session_peak(33), tiled_peak(33)                       # warm-up: packed weights, cache buffers
    staging = 3 * 16 * 64 * 64 * 4                         # one chunk of input frames
    s33, s161 = session_peak(33), session_peak(161)
    t33, t161 = tiled_peak(33), tiled_peak(161)
    assert abs(s161 - s33) < staging, (s33, s161)
    assert t161 - t33 > staging, (t33, t161)                # the same measurement sees the whole-clip path grow


def test_encode_session_push_u8_equals_preprocessed_clip():
    from vidtok_amd.video_io import preprocess_frames

    model, _, _ = _model("vidtok_kl_causal_488_4chn_v1_1")
    frames = torch.randint(0, 256, (23, 72, 96, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(12)).to(DEV)
    ref = model.encode(preprocess_frames(frames, 64, 64))
    s = model.open_encode_session(16)
    zs = [s.push_u8(frames[a:b], 64, 64)[0] for a, b in ((0, 3), (3, 20), (20, 23))]
    zs.append(s.finish()[0])
    assert torch.equal(torch.cat(zs, 2), ref)


# ---- vt_copy_segments ------------------------------------------------------------------------------------------------------
def test_copy_segments_ragged_and_in_graph():
    from vidtok_amd import ops

    g = torch.Generator().manual_seed(13)
    src = torch.randint(0, 256, (1 << 20,), dtype=torch.uint8, generator=g).to(DEV)
    sizes = [1, 3, 15, 16, 17, 31, 64, 100, 4095, 4096, 4097, 65537, 300000]
    offs = [0, 1, 4, 16, 7, 32, 2, 48, 5, 64, 3, 12, 9]          # aligned 16 / 4 / not at all
    dst = torch.zeros(1 << 21, dtype=torch.uint8, device=DEV)
    pairs, ref, s0, d0 = [], torch.zeros_like(dst), 0, 0
    for n, o in zip(sizes, offs):
        a, b = s0 + o, d0 + (o * 3) % 17
        pairs.append((src[a:a + n], dst[b:b + n]))
        ref[b:b + n] = src[a:a + n]
        s0, d0 = a + n + 64, b + n + 64
    table, mx = ops.segment_table(pairs, DEV)
    ops.copy_segments(table, mx)
    assert torch.equal(dst, ref)
    ops.copy_segments(table, 1)                                   # max_bytes only sizes the grid: any value copies everything
    assert torch.equal(dst, ref)
    # inside a graph capture: the replay copies what the sources hold at replay time
    dst.zero_()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            ops.copy_segments(table, mx)
    torch.cuda.synchronize()
    src.copy_(torch.randint(0, 256, (1 << 20,), dtype=torch.uint8, generator=g).to(DEV))
    ref.zero_()
    for s, d in pairs:
        ref[d.data_ptr() - dst.data_ptr():d.data_ptr() - dst.data_ptr() + d.numel()] = s
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dst, ref)


# ---- the C sessions ----------------------------------------------------------------------------------------------------------
def _handle(cfg, sd, dtype):
    from vidtok_amd import lib as L

    lib = L.load()
    prm = cfg["model"]["params"]
    mc = handle_config(L, prm["encoder_config"]["params"], prm["regularizer_config"]["target"], prm["regularizer_config"].get("params", {}),
                       prm["encoder_config"]["target"])
    h = C.c_void_p()
    L.check(lib.vt_create(C.byref(mc), {torch.bfloat16: L.VT_BF16, torch.float32: L.VT_F32}[dtype], C.byref(h)), "vt_create")
    for i in range(lib.vt_weight_count(h)):
        k = lib.vt_weight_name(h, i).decode()
        t = sd[k].detach().float().contiguous().cpu()
        L.check(lib.vt_load_weight(h, k.encode(), t.data_ptr(), (C.c_int64 * t.dim())(*t.shape), t.dim()), "vt_load_weight")
    L.check(lib.vt_prepare(h), "vt_prepare")
    return lib, h, mc


class _CSession:
    def __init__(self, lib, h, kind, B, H, W, c, overlap, cout, Ho, Wo, cap):
        from vidtok_amd import lib as L

        self.lib, self.L = lib, L
        self.s = C.c_void_p()
        L.check(lib.vt_session_create(h, kind, B, H, W, c, int(overlap), C.byref(self.s)), "vt_session_create")
        nb = lib.vt_session_workspace_bytes(self.s)
        assert nb > 0
        self.ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        self.out = torch.empty((B, cout, cap, Ho, Wo), dtype=torch.float32, device=DEV)
        self.cap = cap
        self.pieces = []

    def _st(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def push(self, x):
        n = C.c_int32()
        x = x.contiguous()
        self.L.check(self.lib.vt_session_push(self.s, x.data_ptr(), x.shape[2], self.out.data_ptr(), self.cap, C.byref(n), self.ws.data_ptr(),
                                              self.ws.numel(), self._st()), "vt_session_push")
        self.pieces.append(self.out[:, :, :n.value].clone())

    def finish(self):
        n = C.c_int32()
        self.L.check(self.lib.vt_session_finish(self.s, self.out.data_ptr(), self.cap, C.byref(n), self.ws.data_ptr(), self.ws.numel(),
                                                self._st()), "vt_session_finish")
        self.pieces.append(self.out[:, :, :n.value].clone())
        self.lib.vt_session_destroy(self.s)
        return torch.cat(self.pieces, 2)


def _c_tile(lib, h, mc, x, tc, overlap):
    from vidtok_amd import lib as L

    B, _, T, H, W = x.shape
    f = mc.time_downsample_factor
    tz = lib.vt_tile_latent_frames(h, T, tc)
    ld = (C.c_int32 * 4)()
    L.check(lib.vt_latent_dims(h, T, H, W, ld), "vt_latent_dims")
    nb = lib.vt_tile_workspace_bytes(h, B, T, H, W, tc, int(overlap))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    mom = torch.empty((B, ld[0], tz, ld[2], ld[3]), dtype=torch.float32, device=DEV)
    L.check(lib.vt_tile_encode(h, x.data_ptr(), B, T, H, W, tc, mom.data_ptr(), ws.data_ptr(), nb, st), "vt_tile_encode")
    z = torch.empty((B, mc.z_channels, tz, ld[2], ld[3]), dtype=torch.float32, device=DEV)
    kl = torch.zeros(1, dtype=torch.float32, device=DEV)
    L.check(lib.vt_regularize_kl(h, mom.data_ptr(), None, z.data_ptr(), kl.data_ptr(), B, tz, ld[2], ld[3], st), "vt_regularize_kl")
    dec = torch.empty((B, mc.out_ch, tz * f, H, W), dtype=torch.float32, device=DEV)
    L.check(lib.vt_tile_decode(h, z.data_ptr(), B, tz, ld[2], ld[3], tc // f, int(overlap), dec.data_ptr(), ws.data_ptr(), nb, st), "vt_tile_decode")
    torch.cuda.synchronize()
    return mom, z, dec, ld


def _c_sessions_vs_tile(name, shape, tc, overlap, dtype, splits):
    from vidtok_amd import lib as L

    model, cfg, sd = _model(name, dtype=dtype, c=tc, overlap=overlap)
    lib, h, mc = _handle(cfg, sd, dtype)
    try:
        B, _, T, H, W = shape
        f = mc.time_downsample_factor
        x = _clip(T, seed=14, B=B, hw=H)
        mom, z, dec, ld = _c_tile(lib, h, mc, x, tc, overlap)
        cap_e, cap_d = 64 // f + tc // f + 2, (64 + tc // f + 2) * f
        for split in splits:
            # two encode sessions and two decode sessions on the one handle, their pushes interleaved
            es = [_CSession(lib, h, L.VT_SESSION_ENCODE, B, H, W, tc, False, ld[0], ld[2], ld[3], cap_e) for _ in range(2)]
            ds = [_CSession(lib, h, L.VT_SESSION_DECODE, B, ld[2], ld[3], tc // f, overlap, mc.out_ch, H, W, cap_d) for _ in range(2)]
            t = 0
            for n in split:
                for s in es:
                    s.push(x[:, :, t:t + n])
                t += n
            tz = z.shape[2]
            zsplit = [min(3, tz - a) for a in range(0, tz, 3)]
            t = 0
            for n in zsplit:
                for s in ds:
                    s.push(z[:, :, t:t + n])
                t += n
            for s in es:
                assert torch.equal(s.finish(), mom), split
            for s in ds:
                assert torch.equal(s.finish(), dec), split
        # the Python engine's tiled pass gives the same bits (the handle is the engine)
        z_ref = model.encode(x)
        assert torch.equal(z_ref, z) and torch.equal(model.decode(z_ref), dec)
    finally:
        lib.vt_destroy(h)


def test_c_sessions_equal_tiled_calls():
    _c_sessions_vs_tile("vidtok_kl_causal_488_4chn_v1_1", (1, 3, 39, 64, 64), 16, True, torch.bfloat16, [[39], [1] * 39, [1, 16, 16, 6], [5, 30, 4]])
    _c_sessions_vs_tile("vidtok_kl_causal_488_16chn_v1_1", (2, 3, 29, 64, 64), 8, False, torch.float32, [[2, 13, 14]])


def test_c_session_example_runs(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    exe = os.path.join(str(tmp_path), "session_encode")
    libdir = os.path.join(ROOT, "vidtok_amd")
    cmd = [cc, "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
           os.path.join(ROOT, "examples", "session_encode.c"), "-o", exe, "-L", libdir, "-lvidtok_amd", "-L", "/opt/rocm/lib", "-lamdhip64", "-lm",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout, r.stderr)


# ---- variants tier: BASELINE configs[4] at its stated size -------------------------------------------------------------------
@pytest.mark.variants
def test_configs4_sessions_equal_tiled():
    _c_sessions_vs_tile("vidtok_kl_causal_488_16chn_v1_1", (1, 3, 129, 256, 256), 16, True, torch.bfloat16, [[1] + [16] * 8])
    model, _, _ = _model("vidtok_kl_causal_488_16chn_v1_1", c=16, overlap=True)
    x = _clip(129, seed=15, hw=256)
    z_ref = model.encode(x)
    d_ref = model.decode(z_ref)
    z, _ = _encode(model.open_encode_session(16), x, [1] + [16] * 8)
    assert torch.equal(z, z_ref)
    assert torch.equal(_decode(model.open_decode_session(), z, [4] * 8 + [1]), d_ref)
