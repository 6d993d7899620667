"""Differentiable decode on the GPU: the data-gradient kernels per op against fp64, the whole decoder backward of both causal
families against the oracle's CPU autograd, forward agreement with decode(), determinism, a short training run, one full-size step.

Bounds.  Per op: max|k - ref| / max|ref| <= 1e-5, the bar vt_conv_wgrad is held to with the same arithmetic (exact products of the
rounded operands, fp32 accumulation).  Whole decoder, fp32: 1e-4, what test_backward_host.py allows fp32 autograd on this graph.
Whole decoder, bf16: per parameter twice the distance (relative L2) of the oracle's own CPU bf16-autocast gradients from its fp32
ones, measured in the test.  Every figure is printed before it is asserted.
"""
import dataclasses
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import backward_sites as S  # noqa: E402
from util import build_model, build_oracle, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 11            # decoder_sites' seeds: weights SEED, latent SEED + 1, cotangent SEED + 2


def _mods():
    from vidtok_amd import lib as L
    from vidtok_amd import ops

    return ops, L


def poisoned(t):
    """`t` on the GPU inside a NaN-filled allocation: a kernel reading around its operands shows"""
    n, pad = t.numel(), 64
    flat = torch.full((n + 2 * pad,), float("nan"), dtype=t.dtype, device=DEV)
    v = flat[pad:pad + n].view(t.shape)
    v.copy_(t)
    return v


def ref_dgrad(dy, w5, g, cin, cout, tmode, x_shape):
    """fp64 autograd through backward_sites.virtual_input from the (rounded) operands the kernel reads -> dx NDHWC [.., ld], pad lanes 0"""
    x = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    xv = S.virtual_input(x, g, tmode)[:, :cin]
    y = F.conv3d(xv, w5.double())
    dyc = dy.cpu().double()[..., :cout].permute(0, 4, 1, 2, 3)
    assert y.shape == dyc.shape, (y.shape, dyc.shape)
    (y * dyc).sum().backward()
    return x.grad


def ref_dgrad_taps(dy, w5, g, cin, cout, tmode, x_shape):
    """the same dx tap by tap (one fp64 GEMM per tap, in the style of backward_sites.ref_wgrad_taps): the gradient of the virtual input
    is accumulated window by window, the adjoint of virtual_input (pads, replicate, up-sampling) is taken by autograd of a LINEAR map"""
    dyc = dy.cpu().double()[..., :cout].permute(0, 4, 1, 2, 3)
    B, _, To, Ho, Wo = dyc.shape
    x = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    xv = S.virtual_input(x, g, tmode)[:, :cin]
    dxv = torch.zeros(xv.shape, dtype=torch.float64)
    w = w5.double()
    for a in range(g.kt):
        for p in range(g.kh):
            for q in range(g.kw):
                dxv[:, :, a:a + To, p:p + Ho, q:q + Wo] += torch.einsum("oi,bothw->bithw", w[:, :, a, p, q], dyc)
    (xv * dxv).sum().backward()
    return x.grad


def run_dgrad(dy, w5, g, cin, cout, tmode, dtype, **kw):
    ops, _ = _mods()
    wt = ops.pack_conv_weight_dgrad(w5.float().contiguous().to(DEV), dtype, dy.shape[-1])
    return ops.conv_dgrad(poisoned(dy), poisoned(wt), g, cin=cin, cout=cout, tmode=tmode, **kw)


def check_dgrad(name, dy, w5, g, cin, cout, tmode, dtype, x_shape, full=True, ref_fn=ref_dgrad):
    """one geometry: fp32 dx against fp64, pad lanes, and (full) the bf16 rounding and acc identities"""
    w5 = w5.to(dtype)                         # the rounded weight both sides use
    ref = ref_fn(dy, w5, g, cin, cout, tmode, x_shape)
    dx = run_dgrad(dy, w5, g, cin, cout, tmode, dtype, dx_dtype=torch.float32)
    torch.cuda.synchronize()
    assert tuple(dx.shape) == tuple(x_shape) and dx.dtype == torch.float32
    err = rel_err(dx[..., :cin], ref[..., :cin])
    print(f"[dgrad] {name} {g} tmode {tmode} {dtype}: rel {err:.2e}")
    assert err <= 1e-5, (name, err)
    assert bool((dx[..., cin:] == 0).all()), "pad lanes of dx must be zero"
    if not full:
        return
    acc = torch.randn(x_shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    dxa = run_dgrad(dy, w5, g, cin, cout, tmode, dtype, dx_dtype=torch.float32, acc=acc)
    assert torch.equal(dxa[..., :cin], (dx + acc)[..., :cin]), (name, "acc must equal a separate add bit for bit")
    assert bool((dxa[..., cin:] == 0).all())
    if dtype == torch.bfloat16:
        dxh = run_dgrad(dy, w5, g, cin, cout, tmode, dtype)
        assert dxh.dtype == torch.bfloat16 and torch.equal(dxh, dx.to(torch.bfloat16)), (name, "bf16 dx must be the rounded fp32 dx")
        acch = acc.to(torch.bfloat16)
        dxha = run_dgrad(dy, w5, g, cin, cout, tmode, dtype, acc=acch)
        assert torch.equal(dxha[..., :cin], (dx + acch.float()).to(torch.bfloat16)[..., :cin]), (name, "bf16 dx + acc: one rounding of the fp32 sum")


# ---- 1. per op ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["v1_0", "v1_1"])
def test_conv_dgrad_decoder_sites(key):
    """every convolution site of the decoder, operands as the engine would hand them (garbage in the pad lanes of dy)"""
    torch.set_num_threads(16)
    model, convs, _norms, leaves = S.decoder_sites(key)
    seen = set()
    for site in convs:
        for dtype in (torch.float32, torch.bfloat16):
            x, dy, g, cin, cout, tmode = S.kernel_conv_operands(model, site, dtype)
            w5 = S.weight5(leaves[site.name + ".weight"].detach())
            kind = (g, tmode, cin, cout, tuple(x.shape), dtype)
            check_dgrad(site.name, dy.to(DEV), w5, g, cin, cout, tmode, dtype, tuple(x.shape), full=kind not in seen)
            seen.add(kind)
    assert len(convs) == 65          # every convolution of the decoder (backward_sites: 65 convolution + 54 LayerNorm sites per model)


def test_conv_dgrad_edge_grid():
    """the stride-1 part of backward_sites.edge_geoms (centred time pad, folded up-sampling under a replicate pad, the 2 x 2 phase
    kernels); the strided part is refused with a message"""
    ops, L = _mods()
    B, Ti, Hi, Wi, cin, cout = 2, 3, 5, 6, 12, 20
    gen = torch.Generator().manual_seed(3)
    n_ok = 0
    for name, (g, tmodes) in S.edge_geoms().items():
        for tmode in tmodes:
            To, Ho, Wo = g.out_dims(Ti, Hi, Wi)
            w5 = torch.randn((cout, cin, g.kt, g.kh, g.kw), generator=gen) / (cin * g.kt * g.kh * g.kw) ** 0.5
            for dtype in (torch.float32, torch.bfloat16):
                dy = S.to_ndhwc(torch.randn((B, cout, To, Ho, Wo), generator=gen), ops.pad_channels(cout), dtype, 2).to(DEV)
                if (g.st, g.sh, g.sw) != (1, 1, 1):
                    wt = torch.zeros((cin, g.kt * g.kh * g.kw * dy.shape[-1]), dtype=dtype, device=DEV)
                    with pytest.raises(L.VtError, match="stride"):
                        ops.conv_dgrad(dy, wt, g, cin=cin, cout=cout, tmode=tmode)
                    continue
                check_dgrad(name, dy, w5, g, cin, cout, tmode, dtype, (B, Ti, Hi, Wi, ops.pad_channels(cin)))
                n_ok += 1
    assert n_ok >= 2 * 13


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("with_acc", [False, True], ids=["plain", "acc"])
@pytest.mark.parametrize("ups", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["-", "t", "s", "ts"])
@pytest.mark.parametrize("rep", [0, 2])
def test_grad_fold_grid(rep, ups, with_acc, out_dtype):
    """the finishing kernel of vt_conv_dgrad with one class (stride 1): every fold case bit-equal to torch_backward_ref.grad_fold on the
    same fp32 source.  The kernel adds a pixel's positions frame by frame, the reference folds time first and space second: the source
    holds multiples of 1/16 below 64 and acc integers below 256 (exact in bf16), so every partial sum of the at most 16 + 1 terms is exact
    in fp32 in either order and the results are equal bits -- a wrong address, a lost term or a second rounding is not.  Pad lanes of the
    source hold garbage; those of the result are zero"""
    import torch_backward_ref as BR

    ops, _ = _mods()
    B, Tt, H, W, c, ld = 2, 3, 5, 6, 12, 16
    ut, us = ups
    gen = torch.Generator().manual_seed(100 * rep + 10 * ut + us)
    src = torch.randint(-1023, 1024, (B, rep + (Tt << ut), H << us, W << us, ld), generator=gen).float() / 16
    src[..., c:] = 7.0
    acc = torch.randint(-255, 256, (B, Tt, H, W, ld), generator=gen).float().to(out_dtype) if with_acc else None
    want = BR.grad_fold(src, ups_t=ut, ups_s=us, rep=rep, acc=acc, out_dtype=out_dtype)
    got = ops.grad_fold(src.to(DEV), ups_t=ut, ups_s=us, rep=rep, c=c, acc=None if acc is None else acc.to(DEV), out_dtype=out_dtype)
    assert got.dtype == out_dtype and tuple(got.shape) == (B, Tt, H, W, ld)
    assert torch.equal(got.cpu()[..., :c], want[..., :c])
    assert bool((got[..., c:] == 0).all())


def test_softmax_rows_backward():
    ops, _ = _mods()
    gen = torch.Generator().manual_seed(1)
    Z, Sq, cols, scale = 3, 30, 30, 512 ** -0.5
    for dtype in (torch.float32, torch.bfloat16):
        s = 4 * torch.randn((Z, Sq, cols), generator=gen)
        p = ops.softmax_rows(s.to(DEV), scale, dtype, ld_out=32)
        p[..., cols:] = 7.0                                            # pad columns of P: garbage no result may depend on
        dp = torch.randn((Z, Sq, cols), generator=gen)
        ds = ops.softmax_rows_backward(poisoned(p), poisoned(dp.to(DEV)), scale, cols=cols, ld_out=32)
        pd = p[..., :cols].cpu().double()
        ref = scale * pd * (dp.double() - (dp.double() * pd).sum(-1, keepdim=True))
        err = rel_err(ds[..., :cols], ref)
        print(f"[softmax backward] {dtype} rel {err:.2e}")
        assert err <= (1e-5 if dtype == torch.float32 else 2.0 ** -8)          # bf16: the fp32 row rounded once
        assert bool((ds[..., cols:] == 0).all())
        # the closed form is the softmax's Jacobian: fp64 autograd through softmax(scale * s) of the fp32 case
        if dtype == torch.float32:
            sd = s.double().requires_grad_(True)
            (torch.softmax(scale * sd, -1) * dp.double()).sum().backward()
            assert rel_err(ds[..., :cols], sd.grad) <= 1e-5


def test_transpose_batched():
    ops, _ = _mods()
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn((5, 30, 40), generator=torch.Generator().manual_seed(2)).to(dtype)
        t = ops.transpose_batched(poisoned(x), cols=36, ld_out=32)
        assert tuple(t.shape) == (5, 36, 32) and torch.equal(t[..., :30].cpu(), x[..., :36].transpose(1, 2)) and bool((t[..., 30:] == 0).all())


def test_upsample_mix_forward_backward():
    ops, _ = _mods()
    gen = torch.Generator().manual_seed(4)
    shape, ch = (2, 6, 7, 9, 24), 20
    mf = torch.tensor([0.37])
    a = torch.sigmoid(mf.double())
    for dtype in (torch.float32, torch.bfloat16):
        u, c, dy = (poisoned((1.0 + torch.randn(shape, generator=gen)).to(dtype)) for _ in range(3))
        y = ops.upsample_mix(u, c, mf.to(DEV), ch=ch)
        du, dc, dmix = ops.upsample_mix_backward(dy, u, c, mf.to(DEV), ch=ch)
        ud, cd, dyd = (t.cpu().double()[..., :ch] for t in (u, c, dy))
        tol = 1e-5 if dtype == torch.float32 else 2.0 ** -8
        for got, ref in ((y, a * ud + (1 - a) * cd), (du, a * dyd), (dc, (1 - a) * dyd)):
            assert rel_err(got[..., :ch], ref) <= tol and bool((got[..., ch:] == 0).all())
        ref_mix = (a * (1 - a) * (dyd * (ud - cd)).sum()).item()
        print(f"[mix backward] {dtype}: dmix {dmix.item():.7e} ref {ref_mix:.7e}")
        assert abs(dmix.item() - ref_mix) <= 1e-5 * (dyd * (ud - cd)).abs().sum().item() * float(a * (1 - a))
        du2, dc2, dmix2 = ops.upsample_mix_backward(dy, u, c, mf.to(DEV), ch=ch)
        assert torch.equal(dmix, dmix2)


def test_time_lerp2x_backward():
    ops, _ = _mods()
    gen = torch.Generator().manual_seed(6)
    for Ti in (1, 2, 5):
        for dtype in (torch.float32, torch.bfloat16):
            dy = torch.randn((2, 2 * Ti + 3, 4, 5, 8), generator=gen).to(dtype)
            out = torch.zeros((2, Ti + 1, 4, 5, 8), dtype=dtype, device=DEV)
            ops.time_lerp2x_backward(poisoned(dy), 2, Ti, out, 1)
            x = torch.zeros((2, 8, Ti, 4, 5), dtype=torch.float64, requires_grad=True)
            up = F.interpolate(x, scale_factor=(2.0, 1.0, 1.0), mode="trilinear", align_corners=False) if Ti > 1 else x.repeat_interleave(2, dim=2)
            (up * dy[:, 2:2 + 2 * Ti].double().permute(0, 4, 1, 2, 3)).sum().backward()
            ref = x.grad.permute(0, 2, 3, 4, 1)
            assert rel_err(out[:, 1:], ref) <= (1e-5 if dtype == torch.float32 else 2.0 ** -8) and bool((out[:, :1] == 0).all())
            # and it is the adjoint of the forward kernel: <lerp(x), dy> = <x, lerp^T(dy)>
            if dtype == torch.float32:
                xr = torch.randn((2, Ti, 4, 5, 8), generator=gen).to(DEV)
                lhs = (ops.time_lerp2x(xr).double() * dy[:, 2:2 + 2 * Ti].to(DEV).double()).sum()
                rhs = (xr.double() * out[:, 1:].double()).sum()
                assert abs(lhs - rhs) <= 1e-5 * max(1.0, abs(lhs))


def test_cotangent_layout_and_add():
    ops, _ = _mods()
    g = torch.randn((2, 3, 4, 5, 6), generator=torch.Generator().manual_seed(8))
    for dtype in (torch.float32, torch.bfloat16):
        y = ops.grad_ncthw_to_ndhwc(poisoned(g), dtype, tpad=3)
        assert tuple(y.shape) == (2, 7, 5, 6, 8) and bool((y[:, :3] == 0).all()) and bool((y[..., 3:] == 0).all())
        assert torch.equal(y[:, 3:, ..., :3].cpu(), g.permute(0, 2, 3, 4, 1).to(dtype))
        a, b = poisoned(g.to(dtype)), poisoned((2 * g).to(dtype))
        assert torch.equal(ops.grad_add(a, b), (a.float() + b.float()).to(dtype))


# ---- 2 / 3. the whole decoder -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def oracle_grads(key, autocast=False):
    """the oracle's CPU autograd over the whole decoder with decoder_sites' seeds, plus a requires_grad latent:
    ({name: grad} with "z" for the latent, x_hat)"""
    import oracle.vidtok_oracle as O

    _model, cfg, sd = build_model(S.MODELS[key], seed=SEED)
    eng = build_oracle(cfg, sd)
    leaves = {k: v.detach().float().clone().requires_grad_(True) for k, v in sd.items() if k.startswith("decoder.")}
    z = torch.randn(S.LATENT, generator=torch.Generator().manual_seed(SEED + 1)).requires_grad_(True)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        out = O.decoder_forward(leaves, eng.dec_params, z, eng.version, O.ChunkState())
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(SEED + 2))
    (out.float() * cot).sum().backward()
    g = {k: v.grad for k, v in leaves.items()}
    g["z"] = z.grad
    return g, out.detach().float(), cot


def kernel_grads(key, dtype):
    model, _cfg, _sd = build_model(S.MODELS[key], seed=SEED, device=DEV, dtype=dtype)
    z = torch.randn(S.LATENT, generator=torch.Generator().manual_seed(SEED + 1)).to(DEV).requires_grad_(True)
    out = model.decode_with_grad(z)
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(SEED + 2)).to(DEV)
    (out * cot).sum().backward()
    torch.cuda.synchronize()
    g = {"decoder." + k: p.grad for k, p in model.decoder.named_parameters()}
    g["z"] = z.grad
    return g, out.detach(), model


def k_bias_scale(key):
    """sum |dy| over the pixels of the key projection (largest channel): the scale its bias gradient, a sum that cancels, is judged on"""
    _m, convs, _n, _l = S.decoder_sites(key)
    (site,) = [s for s in convs if s.name.endswith(".attn_1.k.conv")]
    return site.dy.abs().sum(dim=(0, 2, 3, 4)).max().item()


def pclass(name):
    if name == "z" or name.endswith("mix_factor"):
        return name.rsplit(".", 1)[-1]
    kind = "norm" if ".norm" in name else "conv"
    return f"{kind} {name.rsplit('.', 1)[-1]}"


@pytest.mark.parametrize("key", ["v1_0", "v1_1"])
def test_whole_decoder_fp32(key):
    ref, out_ref, _ = oracle_grads(key)
    got, out, _model = kernel_grads(key, torch.float32)
    # every parameter is compared: the site table's set plus the mix factors = every decoder.* key, plus the latent
    leaves = {k for k in ref if k != "z"}
    assert S.expected_parameters(leaves) | {k for k in leaves if k.endswith(".mix_factor")} == leaves == {k for k in got if k != "z"}
    assert sum(k.endswith(".mix_factor") for k in leaves) == 2
    assert rel_err(out, out_ref) <= 1e-3
    worst = {}
    for k in sorted(ref):
        assert got[k] is not None and got[k].shape == ref[k].shape and got[k].dtype == torch.float32, k
        if k.endswith(".attn_1.k.conv.bias"):
            e = (got[k].cpu() - ref[k]).abs().max().item() / k_bias_scale(key)
        else:
            e = rel_err(got[k], ref[k])
        if e >= worst.get(pclass(k), (-1.0, ""))[0]:
            worst[pclass(k)] = (e, k)
    for c, (e, k) in sorted(worst.items()):
        print(f"[whole decoder fp32 {key}] {c}: worst rel {e:.2e} ({k})")
    bad = {c: v for c, v in worst.items() if v[0] > 1e-4}
    assert not bad, bad


@pytest.mark.parametrize("key", ["v1_0", "v1_1"])
def test_whole_decoder_bf16(key):
    """bf16 kernels against the fp32 reference; the margin is twice what the oracle itself loses under CPU bf16 autocast"""
    ref, _out, _ = oracle_grads(key)
    ref16, _o16, _ = oracle_grads(key, True)
    got, _o, _model = kernel_grads(key, torch.bfloat16)

    def l2(a, b):
        return ((a.double().cpu() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()

    bad = []
    for k in sorted(ref):
        if k.endswith(".attn_1.k.conv.bias"):
            # a sum of terms that cancels: each term carries bf16 rounding (2^-9 relative), so what is left is bounded by 2^-9 sum|dy|;
            # a factor 4 for the chain of rounded tensors dK is computed from
            e, allow = got[k].abs().max().item() / k_bias_scale(key), 4 * 2.0 ** -9
            own = ref16[k].abs().max().item() / k_bias_scale(key)
        else:
            own = l2(ref16[k], ref[k])
            e, allow = l2(got[k], ref[k]), 2 * own
        print(f"[whole decoder bf16 {key}] {k}: kernels {e:.3e}, oracle under autocast {own:.3e}, allowed {allow:.3e}")
        if not e <= allow:
            bad.append((k, e, allow))
    assert not bad, bad


# ---- 4. forward agreement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["v1_0", "v1_1"])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-3), (torch.bfloat16, 5e-2)])
def test_forward_agrees_with_decode(key, dtype, tol):
    model, _cfg, _sd = build_model(S.MODELS[key], seed=SEED, device=DEV, dtype=dtype)
    z = torch.randn((1, 4, 3, 8, 8), generator=torch.Generator().manual_seed(1)).to(DEV)
    a, b = model.decode_with_grad(z), model.decode(z)
    assert a.shape == b.shape and a.dtype == torch.float32 and not b.requires_grad
    assert a.requires_grad and a.grad_fn is not None             # the decoder's parameters ask for gradients
    a2 = model.decode_with_grad(z.clone().requires_grad_(True))
    assert a2.requires_grad and torch.equal(a2, a)
    for p in model.decoder.parameters():
        p.requires_grad_(False)
    assert not model.decode_with_grad(z).requires_grad           # nobody asks: no graph
    e = rel_err(a, b)
    print(f"[forward agreement {key} {dtype}] rel {e:.2e}")
    assert e <= tol
    with torch.autocast("cuda", dtype=torch.bfloat16):           # the caller's autocast region selects the bf16 kernels
        c = model.decode_with_grad(z)
    assert rel_err(c, b) <= 5e-2


# ---- 5. determinism -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_runs_give_the_same_bits(dtype):
    a, oa, _ = kernel_grads("v1_1", dtype)
    b, ob, _ = kernel_grads("v1_1", dtype)
    assert torch.equal(oa, ob)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- 6. it trains -----------------------------------------------------------------------------------------------------------------------
def test_five_sgd_steps_and_graph_recapture():
    model, _cfg, _sd = build_model(S.MODELS["v1_0"], seed=5, device=DEV, dtype=torch.float32)
    x = (torch.rand((1, 3, 9, 32, 32), generator=torch.Generator().manual_seed(0)) * 2 - 1).to(DEV)
    torch.manual_seed(1)
    z = model.encode(x)                                          # the frozen encoder: no_grad, as it stays
    assert not z.requires_grad
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.enable_graphs()
    old = [model.decode(z) for _ in range(3)][-1].clone()        # captured against the initial weights
    opt = torch.optim.SGD(model.decoder.parameters(), lr=2e-3)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = F.mse_loss(model.decode_with_grad(z), x)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    losses.append(F.mse_loss(model.decode(z), x).item())
    print("[training] losses", " ".join(f"{v:.6f}" for v in losses))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    graphed = [model.decode(z) for _ in range(3)][-1].clone()
    model.enable_graphs(False)
    eager = model.decode(z)
    assert torch.equal(graphed, eager) and not torch.equal(graphed, old)      # the parameter-version fingerprint forced a recapture
    after = model.state_dict()
    changed = {k for k in before if not torch.equal(before[k], after[k])}
    assert all(k.startswith("decoder.") for k in changed), sorted(changed)[:5]
    assert "decoder.conv_out.conv.weight" in changed and sum(k.endswith(".mix_factor") for k in changed) == 2


# ---- 7. size ----------------------------------------------------------------------------------------------------------------------------
def test_full_size_step_bf16():
    model, _cfg, _sd = build_model(S.MODELS["v1_0"], seed=5, device=DEV, dtype=torch.bfloat16)
    x = (torch.rand((1, 3, 17, 256, 256), generator=torch.Generator().manual_seed(0)) * 2 - 1).to(DEV)
    z = model.encode(x).requires_grad_(True)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = F.mse_loss(model.decode_with_grad(z), x)
    loss.backward()
    torch.cuda.synchronize()
    print(f"[full size] 1x17x256x256 bf16: loss {loss.item():.5f}, peak memory of forward + backward {(torch.cuda.max_memory_allocated() - base) / 2 ** 30:.2f} GiB "
          f"over {base / 2 ** 30:.2f} GiB resident")
    assert bool(torch.isfinite(z.grad).all())
    for k, p in model.decoder.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k


@pytest.mark.parametrize("name,g,rep,cin,cout,xs", [
    ("resnet 3x3 128->128 at 256 x 256", dict(kh=3, kw=3, ph=1, pw=1, ph_hi=1, pw_hi=1), False, 128, 128, (1, 2, 256, 256)),
    ("temporal k3 256->256 replicate at 128 x 128", dict(kt=3, pt=2), True, 256, 256, (1, 6, 128, 128)),
    ("upsample 3x3 256->256 to 128 x 128", dict(kh=3, kw=3, ph=1, pw=1, ph_hi=1, pw_hi=1, ups_s=1), False, 256, 256, (1, 2, 64, 64)),
])
def test_large_sites_against_taps(name, g, rep, cin, cout, xs):
    ops, L = _mods()
    torch.set_num_threads(16)
    g = ops.ConvGeom(**g)
    tmode = L.VT_TPAD_REPLICATE if rep else L.VT_TPAD_ZERO
    gen = torch.Generator().manual_seed(9)
    To, Ho, Wo = g.out_dims(*xs[1:])
    w5 = torch.randn((cout, cin, g.kt, g.kh, g.kw), generator=gen) / (cin * g.kt * g.kh * g.kw) ** 0.5
    dy = torch.randn((xs[0], To, Ho, Wo, cout), generator=gen).to(torch.bfloat16).to(DEV)
    check_dgrad(name, dy, w5, g, cin, cout, tmode, torch.bfloat16, (xs[0],) + tuple(xs[1:]) + (cin,), ref_fn=ref_dgrad_taps)
