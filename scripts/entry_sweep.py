"""One call of every pointwise / backward entry point per storage type it serves, on seeded inputs: one sha256 per output tensor.

    python scripts/entry_sweep.py [> digests.txt]                       the in-tree library (or VIDTOK_AMD_LIB=PATH)
    python scripts/entry_sweep.py --compare A.txt B.txt                 the rows that differ between two runs
    rocprofv3 --kernel-trace --output-format csv -- python scripts/entry_sweep.py
    python scripts/entry_sweep.py --geometry TRACE_A.csv TRACE_B.csv    (kernel, grid, workgroup, LDS) sequences of two traces

A tool for A/B runs of two builds of the library whose host code differs (csrc/launch.h and the files on it): equal digests say the
same kernels got the same arguments, equal trace rows say no grid, block or LDS size moved.  Shapes: those of the entry points' GPU
tests, plus ragged ones (1031 rows at C = 3 / ld = 8 and C = 64; 8 * 1031 elements; B 2, C 3, T 3, H 5, W 7, tpad 2) where a test
shape fits one workgroup or divides the block span: the last workgroup is partial and the fixed-order partial sums depend on the grid.
Entry points that add with float atomics (vt_eval_psnr_ssim, vt_fsq_aux_stats, the frame / clip scopes of vt_groupnorm_act) are not bit-reproducible
from run to run; their rows are marked `~` and --compare lists them apart.  Needs a GPU; a few seconds."""
import csv
import hashlib
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M_RAGGED = 1031


def sweep(emit):
    import torch

    from vidtok_amd import lib as L
    from vidtok_amd import ops

    dev = "cuda:0"
    g = torch.Generator().manual_seed(20240229)
    f32, bf16, f16 = torch.float32, torch.bfloat16, torch.float16

    def rnd(*shape, dtype=f32, lo=-1.0, hi=1.0):
        return (torch.rand(shape, generator=g) * (hi - lo) + lo).to(dtype).to(dev)

    def padded(rows, c, ld, dtype):               # [rows, ld] with the channels past c zero
        t = torch.zeros(rows, ld)
        t[:, :c] = torch.rand(rows, c, generator=g) * 2 - 1
        return t.to(dtype).to(dev)

    # ---- pointwise.hip
    for ti, to in ((f32, f32), (bf16, bf16), (f32, bf16), (bf16, f32), (f16, f16), (f32, f16), (f16, f32)):
        for c in (32, 64, 128, 192, 256, 512, 1024, 2048):      # every (LP, R) instantiation
            x = rnd(2, 3, 5, 7, c, dtype=ti)
            emit(f"layernorm_act {ti}->{to} C={c}", ops.layernorm_act(x, rnd(c), rnd(c), silu=c != 64, out_dtype=to))
        emit(f"layernorm_act {ti}->{to} rows={M_RAGGED}", ops.layernorm_act(rnd(M_RAGGED, 64, dtype=ti), rnd(64), rnd(64), silu=True, out_dtype=to))
    emit("tanh_inplace", ops.tanh_(rnd(8 * M_RAGGED, lo=-3, hi=3)))
    for dt in (f32, bf16, f16):
        emit(f"softmax_rows {dt}", ops.softmax_rows(rnd(M_RAGGED, 45, lo=-4, hi=4), 0.125, dt, ld_out=48))
        emit(f"ncthw_to_ndhwc {dt}", ops.ncthw_to_ndhwc(rnd(2, 3, 3, 5, 7), dt, tpad=2), ops.ncthw_to_ndhwc(rnd(1, 3, 5, 32, 48), dt))
        emit(f"ndhwc_to_ncthw {dt}", ops.ndhwc_to_ncthw(rnd(2, 5, 5, 7, 8, dtype=dt), 3, ttrim=2), ops.ndhwc_to_ncthw(rnd(1, 5, 32, 48, 8, dtype=dt), 3))
        for tmode in (L.VT_TPAD_ZERO, L.VT_TPAD_REPLICATE, L.VT_TPAD_CACHE, L.VT_TPAD_ZERO_BACK):
            x = rnd(2, 5, 5, 7, 8, dtype=dt)
            emit(f"time_avgpool3s2 {dt} tmode={tmode}", ops.time_avgpool3s2(x, tmode, cache=rnd(2, 1, 5, 7, 8, dtype=dt) if tmode == L.VT_TPAD_CACHE else None))
        emit(f"time_avgpool3s2 {dt} big", ops.time_avgpool3s2(rnd(1, 4, M_RAGGED, 1, 8, dtype=dt)))
        emit(f"time_lerp2x {dt}", ops.time_lerp2x(rnd(2, 3, 5, 7, 8, dtype=dt)), ops.time_lerp2x(rnd(1, 2, M_RAGGED, 1, 8, dtype=dt)))
        emit(f"time_lerp2x_cat {dt}", ops.time_lerp2x_cat(rnd(2, 1, 5, 7, 8, dtype=dt), rnd(2, 2, 5, 7, 8, dtype=dt), 2))
        emit(f"gather_frames {dt}", ops.gather_frames(rnd(2, 4, 5, 7, 8, dtype=dt), [3, 0, 0, 2]), ops.gather_frames(rnd(2, 3, 5, 7, 3, dtype=dt)[..., :2].contiguous(), [2, 1]))
    # ---- groupnorm.hip
    for ti, to in ((f32, f32), (bf16, bf16), (f32, bf16), (bf16, f32), (f16, f16), (f32, f16), (f16, f32)):
        x = rnd(2, 3, 5, 7, 64, dtype=ti)
        emit(f"groupnorm_act pixel {ti}->{to}", ops.groupnorm_act(x, rnd(64), rnd(64), scope=L.VT_GN_PIXEL, silu=True, out_dtype=to))
        for scope in (L.VT_GN_FRAME, L.VT_GN_CLIP):
            emit(f"~groupnorm_act scope={scope} {ti}->{to}", ops.groupnorm_act(x, rnd(64), rnd(64), scope=scope, silu=False, out_dtype=to))
    # ---- regularizers.hip
    emit("kl_sample", *ops.kl_sample(rnd(2, 8, 3, 5, 7), rnd(2, 4, 3, 5, 7)))
    levels = [8, 8, 8, 5, 5, 5]
    for ncb in (1, 2):
        z, idx = ops.fsq_quantize(rnd(2, 6 * ncb, 3, 5, 7, lo=-2, hi=2), levels, ncb)
        emit(f"fsq_quantize ncb={ncb}", z, idx)
        emit(f"fsq_indices_to_codes ncb={ncb}", ops.fsq_indices_to_codes(idx, levels, ncb))
    emit("fsq_quantize big", *ops.fsq_quantize(rnd(1, 6, 8 * M_RAGGED, lo=-2, hi=2), levels))
    emit("channel_linear", ops.channel_linear(rnd(2, 6, 3, 5, 7), rnd(4, 6), rnd(4)), ops.channel_linear(rnd(1, 4, M_RAGGED), rnd(6, 4), None))
    st, avg = ops.fsq_aux_stats(rnd(2, 4, 3, 5, 7, lo=-2, hi=2), [8, 5, 5, 5], return_avg=True)
    emit("~fsq_aux_stats", st, avg)
    emit("entropy", ops.entropy(torch.softmax(rnd(1000), 0)).reshape(1))
    emit("fsq_aux_loss", ops.fsq_aux_loss(rnd(3), None, 1.0, 0.1, 0.25).reshape(1), ops.fsq_aux_loss(rnd(3), rnd(1), 1.0, 0.1, 0.25).reshape(1))
    # ---- metrics.hip, video_io.hip, segments.hip, packing.hip
    emit("~eval_psnr_ssim", *ops.eval_psnr_ssim(rnd(1, 3, 2, 40, 56), rnd(1, 3, 2, 40, 56)))
    frames = (torch.rand(3, 37, 53, 3, generator=g) * 255).to(torch.uint8).to(dev)
    x = ops.frames_u8_to_ncthw(frames, (24, 34), (1, 2), (20, 28))
    emit("frames_u8_to_ncthw", x)
    emit("ncthw_to_frames_u8", ops.ncthw_to_frames_u8(x, 1, 2))
    emit("ncthw_copy_frames", ops.ncthw_copy_frames(rnd(2, 3, 4, 5, 7, lo=-2, hi=2), torch.zeros(2, 3, 5, 5, 7, device=dev), 1, 2, 3, clamp=True))
    srcs = [rnd(n, dtype=dt) for n, dt in ((8 * M_RAGGED, f32), (7, bf16), (64, f32), (1 << 18, bf16))]
    dsts = [torch.zeros_like(s) for s in srcs]
    table, mx = ops.segment_table(list(zip(srcs, dsts)), dev)
    ops.copy_segments(table, mx)
    emit("copy_segments", *dsts)
    w = rnd(24, 5, 3, 3, 3)
    for dt in (f32, bf16, f16):
        emit(f"pack_conv_weight {dt}", ops.pack_conv_weight(w, dt), ops.pack_conv_weight(w[:, :, 0].contiguous(), dt, mix=[[0, 1, 3, 4], [2, 5, -1, -1], [6, -1, 7, -1], [8, -1, -1, -1]]))
    emit("pack_conv_weight split3", ops.pack_conv_weight(w, f32, split3=True))
    # ---- lpips.hip
    shift, scale = rnd(3, lo=-0.1, hi=0.1), rnd(3, lo=0.2, hi=0.5)
    for dt in (f32, bf16, f16):
        emit(f"lpips_prep {dt}", ops.lpips_prep(rnd(1, 3, 2, 17, 19), rnd(1, 3, 2, 17, 19, lo=-1.5, hi=1.5), shift, scale, dt, flags=L.VT_LPIPS_CLAMP_Y | L.VT_LPIPS_ROUNDTRIP))
        n = 2
        work = torch.zeros(5 * n * 64, dtype=f32, device=dev)
        for tap, (c, h, wd) in enumerate(((64, 16, 16), (128, 9, 11), (256, 5, 7), (512, 5, 5), (512, 37, 41))):
            emit(f"lpips_tap {dt} C={c}", ops.lpips_tap(rnd(2 * n, h, wd, c, dtype=dt, lo=0, hi=1), rnd(c, lo=0, hi=1), work, tap))
        emit(f"lpips_finish after {dt}", work, *ops.lpips_finish(work, n, 16, 16, tap_means=True))
    # ---- lpips_grad.hip
    for dt, dd in ((f32, f32), (bf16, f32), (bf16, bf16)):
        for c, h, wd in ((64, 16, 16), (128, 9, 11), (256, 5, 7), (512, 5, 5), (64, 75, 83)):
            feat = rnd(4, h, wd, c, dtype=dt, lo=-0.5, hi=1)
            emit(f"lpips_tap_backward {dt} dpool {dd} C={c} {h}x{wd}", ops.lpips_tap_backward(feat, rnd(c, lo=0, hi=1), rnd(2), rnd(2, h // 2, wd // 2, c, dtype=dd)),
                 ops.lpips_tap_backward(feat, rnd(c, lo=0, hi=1), rnd(2), None))
        emit(f"relu_backward {dt} dy {dd}", ops.relu_backward(rnd(8 * M_RAGGED, dtype=dd), rnd(8 * M_RAGGED, dtype=dt)))
        emit(f"leaky_relu_backward {dt} dy {dd}", ops.leaky_relu_backward(rnd(8 * M_RAGGED, dtype=dd), rnd(8 * M_RAGGED, dtype=dt), 0.2))
    for dt in (f32, bf16):
        emit(f"lpips_prep_backward {dt}", ops.lpips_prep_backward(rnd(2, 17, 19, 8, dtype=dt), scale), ops.lpips_prep_backward(rnd(1, M_RAGGED, 5, 8, dtype=dt), scale))
    # ---- grad.hip
    G = ops.ConvGeom
    for dt in (f32, bf16):
        for geom, tmode in ((G(3, 3, 3, pt=2, ph=1, pw=1, ph_hi=1, pw_hi=1), L.VT_TPAD_REPLICATE), (G(1, 3, 3, sh=2, sw=2, ph_hi=1, pw_hi=1), L.VT_TPAD_ZERO),
                            (G(3, 3, 3, pt=2, ph=1, pw=1, ph_hi=1, pw_hi=1, ups_t=1, ups_s=1), L.VT_TPAD_ZERO)):
            x = padded(2 * 3 * 9 * 11, 5, 8, dt).reshape(2, 3, 9, 11, 8)
            dy = padded(2 * 9 * 11 * 3 * 8, 12, 16, dt)
            dy = dy[:2 * math.prod(geom.out_dims(3, 9, 11))].reshape(2, *geom.out_dims(3, 9, 11), 16)
            emit(f"conv_wgrad {dt} {geom}", *ops.conv_wgrad(x, dy, geom, cin=5, cout=12, tmode=tmode))
        for dd in ((f32,) if dt == f32 else (f32, bf16)):
            for c, ld, rows in ((3, 8, M_RAGGED), (64, 64, M_RAGGED), (128, 128, 70), (192, 192, 70), (256, 256, 70), (512, 512, 33)):
                emit(f"layernorm_act_backward {dt}->{dd} C={c}", *ops.layernorm_act_backward(padded(rows, c, ld, dt), padded(rows, c, ld, dt), rnd(c), rnd(c), silu=c != 128, c=c, dx_dtype=dd))
    # ---- grad_decoder.hip
    for dt in (f32, bf16):
        wt = rnd(12, 5, 3, 3, 3)
        for geom, tmode, in_hw in ((G(3, 3, 3, pt=2, ph=1, pw=1, ph_hi=1, pw_hi=1), L.VT_TPAD_REPLICATE, None), (G(3, 3, 3, pt=2, ph=1, pw=1, ph_hi=1, pw_hi=1), L.VT_TPAD_ZERO, None),
                                   (G(3, 3, 3, pt=2, ph=1, pw=1, ph_hi=1, pw_hi=1, ups_t=1, ups_s=1), L.VT_TPAD_ZERO, None), (G(1, 3, 3, sh=2, sw=2, ph_hi=1, pw_hi=1), L.VT_TPAD_ZERO, (9, 11))):
            wsrc = wt if geom.kt == 3 else wt[:, :, :1].contiguous()
            strided = geom.sh > 1
            pk = ops.pack_conv_weight_dgrad(wsrc, dt, 16, geom if strided else None)
            emit(f"pack_conv_weight_dgrad {dt} {geom}", pk)
            hi, wi = (9, 11) if strided or geom.ups_s == 0 else (5, 6)
            ti_ = 3 if geom.ups_t == 0 else 2
            od = geom.out_dims(ti_, hi, wi)
            dy = padded(2 * od[0] * od[1] * od[2], 12, 16, dt).reshape(2, *od, 16)
            for dd in ((f32,) if dt == f32 else (f32, bf16)):
                acc = padded(2 * ti_ * hi * wi, 5, 8, dd).reshape(2, ti_, hi, wi, 8)
                emit(f"conv_dgrad {dt}->{dd} {geom} tmode={tmode}", ops.conv_dgrad(dy, pk, geom, cin=5, cout=12, tmode=tmode, acc=acc, dx_dtype=dd, in_hw=in_hw),
                     ops.conv_dgrad(dy, pk, geom, cin=5, cout=12, tmode=tmode, dx_dtype=dd, in_hw=in_hw))
        for src_dt in ((f32,) if dt == f32 else (f32, bf16)):
            emit(f"grad_fold {src_dt}->{dt}", ops.grad_fold(rnd(2, 2 + 6, 10, 14, 8, dtype=src_dt), ups_t=1, ups_s=1, rep=2, c=3, acc=rnd(2, 3, 5, 7, 8, dtype=dt), out_dtype=dt),
                 ops.grad_fold(rnd(1, 2, M_RAGGED, 1, 8, dtype=src_dt), ups_t=1, out_dtype=dt))
        p = torch.softmax(rnd(M_RAGGED, 45, lo=-3, hi=3), -1)
        emit(f"softmax_rows_backward {dt}", ops.softmax_rows_backward(torch.nn.functional.pad(p, (0, 3)).to(dt).to(dev), rnd(M_RAGGED, 45), 0.125, cols=45))
        emit(f"transpose_batched {dt}", ops.transpose_batched(rnd(3, 45, 72, dtype=dt), cols=70))
        mf = rnd(1)
        u, c_, dyy = (padded(M_RAGGED, 3, 8, dt) for _ in range(3))
        emit(f"upsample_mix {dt}", ops.upsample_mix(u, c_, mf, ch=3), ops.upsample_mix(rnd(70, 64, dtype=dt), rnd(70, 64, dtype=dt), mf))
        emit(f"upsample_mix_backward {dt}", *ops.upsample_mix_backward(dyy, u, c_, mf, ch=3), *ops.upsample_mix_backward(rnd(4 * M_RAGGED, 64, dtype=dt), rnd(4 * M_RAGGED, 64, dtype=dt), rnd(4 * M_RAGGED, 64, dtype=dt), mf))
        emit(f"time_lerp2x_backward {dt}", ops.time_lerp2x_backward(rnd(2, 8, 5, 7, 8, dtype=dt), 2, 3, torch.zeros(2, 4, 5, 7, 8, dtype=dt, device=dev), 1))
        emit(f"grad_ncthw_to_ndhwc {dt}", ops.grad_ncthw_to_ndhwc(rnd(2, 3, 3, 5, 7), dt, tpad=2), ops.grad_ncthw_to_ndhwc(rnd(1, 3, 2, 32, 48), dt))
        emit(f"grad_add {dt}", ops.grad_add(rnd(8 * M_RAGGED, dtype=dt), rnd(8 * M_RAGGED, dtype=dt)))
    # ---- patchgan.hip
    for dt in (f32, bf16):
        for c, ld, rows in ((3, 8, M_RAGGED), (64, 64, M_RAGGED), (512, 512, 70)):
            x = padded(rows, c, ld, dt)
            mean, var, rstd = ops.batchnorm_stats(x, c)
            emit(f"batchnorm_stats {dt} C={c}", mean, var, rstd)
            gm, bt = rnd(c), rnd(c)
            emit(f"batchnorm_act {dt} C={c}", ops.batchnorm_act(x, mean, rstd, gm, bt, 0.2, c))
            for dd in ((f32,) if dt == f32 else (f32, bf16)):
                for batch in (True, False):
                    emit(f"batchnorm_act_backward {dt} dy {dd} C={c} batch={batch}", *ops.batchnorm_act_backward(x, padded(rows, c, ld, dd), mean, rstd, gm, bt, 0.2, batch=batch, c=c))
    torch.cuda.synchronize()


def run():
    import torch

    def emit(label, *tensors):
        for i, t in enumerate(tensors):
            raw = t.detach().reshape(-1).contiguous().cpu().view(torch.uint8).numpy().tobytes()
            print(f"{label} [{i}] {tuple(t.shape)} {hashlib.sha256(raw).hexdigest()}")

    sweep(emit)


def compare(a, b):
    ra, rb = ([ln.rstrip("\n") for ln in open(p) if "] (" in ln] for p in (a, b))
    if [r.rsplit(" ", 1)[0] for r in ra] != [r.rsplit(" ", 1)[0] for r in rb]:
        print(f"the two runs hold different rows ({len(ra)} / {len(rb)})")
        return 1
    diff = [x for x, y in zip(ra, rb) if x != y]
    hard = [x for x in diff if not x.startswith("~")]
    soft = sum(x.startswith("~") for x in ra)
    print(f"{len(ra)} digests, {len(ra) - soft} of reproducible entry points: {len(hard)} differ; {soft} of entry points with float atomics (~): {len(diff) - len(hard)} differ")
    for x in diff[:20]:
        print("  differs:", x.rsplit(" ", 1)[0])
    return 1 if hard else 0


def geometry(a, b):
    def rows(path):
        with open(path, newline="") as f:
            rd = list(csv.DictReader(f))
        rd.sort(key=lambda r: int(r["Start_Timestamp"]))
        keys = ("Kernel_Name", "Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z", "LDS_Block_Size", "Scratch_Size")
        return [tuple(r.get(k, "") for k in keys) for r in rd]

    ra, rb = rows(a), rows(b)
    bad = [(i, x, y) for i, (x, y) in enumerate(zip(ra, rb)) if x != y]
    print(f"{len(ra)} / {len(rb)} kernel launches, {len(set(r[0] for r in ra))} distinct kernels: {len(bad)} rows differ")
    for i, x, y in bad[:10]:
        print(f"  launch {i}: {x} | {y}")
    return 1 if bad or len(ra) != len(rb) else 0


if __name__ == "__main__":
    if "--compare" in sys.argv:
        sys.exit(compare(*sys.argv[sys.argv.index("--compare") + 1:][:2]))
    if "--geometry" in sys.argv:
        sys.exit(geometry(*sys.argv[sys.argv.index("--geometry") + 1:][:2]))
    run()
