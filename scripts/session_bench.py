"""Streaming sessions vs the whole-clip tiled path on BASELINE.json configs[4] (vidtok_kl_causal_488_16chn_v1_1, bf16, one clip
of 129 x 256 x 256, t_chunk_enc 16, decoder look-ahead, chunk graphs on):

  * encode / decode frames/s: tile_encode / tile_decode of the clip on the device vs an encode session fed 16-frame pushes and a
    decode session fed 4-latent pushes (the input slices are already on the device: the kernels are compared, not the upload);
  * the cost of a session switch: the state of one session copied into the model's cache buffers and back out (two
    vt_copy_segments launches) vs the same copies as one torch copy per cache tensor;
  * the peak device memory (torch.cuda.max_memory_allocated above what was allocated before) of an encode + decode session pair
    over 129 and 1 025 frames pushed from the host, against the tiled forward of the same clips on the device.

    python scripts/session_bench.py [--out profiles/session_bench.json] [--steps 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps, warmup=1):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from util import build_model

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--long", type=int, default=1025)
    a = ap.parse_args()
    dev = "cuda:0"
    name = "vidtok_v1_1/vidtok_kl_causal_488_16chn_v1_1"
    model, _, _ = build_model(name, seed=0, device=dev, dtype=torch.bfloat16)
    model.regularization.sample = False
    model.use_tiling, model.t_chunk_enc, model.t_chunk_dec, model.use_overlap = True, 16, 4, True
    model.enable_graphs(True)
    T, R = 129, 256
    x = (torch.rand((1, 3, T, R, R), generator=torch.Generator().manual_seed(2)) * 2 - 1).to(dev)
    pieces = [x[:, :, 0:1].contiguous()] + [x[:, :, a:a + 16].contiguous() for a in range(1, T, 16)]
    z = model.encode(x)
    zp = [z[:, :, a:a + 4].contiguous() for a in range(0, z.shape[2], 4)]
    out = {"box": torch.cuda.get_device_name(0), "workload": f"{name}, bf16, 1 x {T} x {R} x {R}, t_chunk_enc 16, look-ahead, graphs on",
           "unit": "frames/s"}

    def sess_encode():
        s = model.open_encode_session(16)
        for p in pieces:
            s.push(p)
        return s.finish()

    def sess_decode():
        s = model.open_decode_session(4, True)
        for p in zp:
            s.push(p)
        return s.finish()

    t_te = timed(lambda: model.encode(x), a.steps)
    t_se = timed(sess_encode, a.steps)
    t_td = timed(lambda: model.decode(z), a.steps)
    t_sd = timed(sess_decode, a.steps)
    out["encode"] = {"tile_encode": round(T / t_te, 2), "session_16_frame_pushes": round(T / t_se, 2), "session_vs_tiled": round(t_te / t_se, 4)}
    out["decode"] = {"tile_decode": round(T / t_td, 2), "session_4_latent_pushes": round(T / t_sd, 2), "session_vs_tiled": round(t_td / t_sd, 4)}

    # the switch: one session with state, in and out of the model (_enter / _leave / _restore: what every push adds)
    s = model.open_encode_session(16)
    s.push(pieces[0])
    s.push(pieces[1])
    n_caches = sum(t is not None for t in s._saved)
    cache_bytes = sum(t.numel() * t.element_size() for t in s._saved if t is not None)

    def switch():
        s._enter()
        s._leave()
        s._restore()

    def switch_torch():                       # the same bytes as one torch copy per cache tensor, both ways
        bufs = [slot.cache for slot in s.state.slots]
        for sv, b in zip(s._saved, bufs):
            if sv is not None and b is not None:
                b.copy_(sv)
        for sv, b in zip(s._saved, bufs):
            if sv is not None and b is not None:
                sv.copy_(b)

    def switch_segments():                    # the device part of a switch alone: the two vt_copy_segments launches
        bufs = [slot.cache for slot in s.state.slots]
        s._copy([(sv, b) for sv, b in zip(s._saved, bufs) if sv is not None and b is not None])
        s._copy([(b, sv) for sv, b in zip(s._saved, bufs) if sv is not None and b is not None])

    n = 100
    t_sw = timed(switch, n, warmup=5)
    s._enter()
    try:
        t_seg = timed(switch_segments, n, warmup=5)
        t_sw_torch = timed(switch_torch, n, warmup=5)
    finally:
        s._leave()
        s._restore()
    out["switch"] = {"caches": n_caches, "cache_bytes": cache_bytes, "us_per_switch": round(t_sw * 1e6, 2),
                     "us_two_copy_segments": round(t_seg * 1e6, 2), "us_torch_copy_per_tensor": round(t_sw_torch * 1e6, 2),
                     "GBps_copy_segments": round(2 * 2 * cache_bytes / t_seg / 1e9, 1),
                     "note": "us_per_switch: wall time of what a push adds (state in + out, snapshot / restore of the chunk states); "
                             "the other two: the same 2 x cache_bytes moved as two vt_copy_segments launches vs one torch copy per tensor; "
                             "GBps counts bytes read + written"}

    # peak device memory vs length
    def sess_peak(Tn):
        xs = torch.rand((1, 3, 16, R, R), generator=torch.Generator().manual_seed(3)) * 2 - 1      # the same 16 frames, pushed again and again
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        rs = model.open_reconstruct_session()
        left = Tn
        first = True
        while left:
            k = 1 if first else min(16, left)
            o = rs.push(xs[:, :, :k].to(dev))
            if o is not None:
                o.cpu()
            left -= k
            first = False
        rs.finish()[0].cpu()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    def tiled_peak(Tn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        xl = (torch.rand((1, 3, Tn, R, R), generator=torch.Generator().manual_seed(4)) * 2 - 1).to(dev)
        model(xl)[1].cpu()
        del xl
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    sess_peak(33)
    mem = {}
    for Tn in (T, a.long):
        mem[str(Tn)] = {"session_MiB": round(sess_peak(Tn) / 2**20, 1), "tiled_forward_MiB": round(tiled_peak(Tn) / 2**20, 1)}
    out["peak_memory_reconstruct"] = mem
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
