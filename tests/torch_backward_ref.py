"""TEST INFRASTRUCTURE ONLY -- plain PyTorch statements of the backward operators of vidtok_amd.ops (the differentiable decode),
with the same Python signatures, for host-logic tests of vidtok_amd/backward.py on a machine without a GPU.

Each one is the closed form of the gradient of the forward statement of tests/torch_ops_ref.py (torch's own convolution backward for
the two convolution gradients) on the stored operands, computed in fp32 and rounded once to the dtype the kernel would write; none of
them enters the autograd engine, so they can run inside an autograd.Function's backward.  `patched_ops()` swaps them, together with the forward statements, in
for vidtok_amd.ops.  The product never imports this file.
"""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import backward_sites as S
import torch_ops_ref as R
from vidtok_amd import lib as L
from vidtok_amd.ops import pad_channels


def _k3(weight):
    return (weight.shape[2], 1, 1) if weight.dim() == 3 else (1,) * (5 - weight.dim()) + tuple(weight.shape[2:])


def pack_conv_weight_dgrad(weight, dtype, cout_stored=None):
    cout, cin = weight.shape[:2]
    w5 = weight.detach().float().reshape((cout, cin) + _k3(weight))
    r = w5.flip(2, 3, 4).permute(1, 2, 3, 4, 0)                                       # [cin, kt, kh, kw, cout]
    return F.pad(r, (0, (cout_stored or pad_channels(cout)) - cout)).reshape(cin, -1).to(dtype).contiguous()


def _virtual(x, geom, tmode, cin):
    return S.virtual_input(x.float()[..., :cin], geom, tmode)


def conv_wgrad(x, dy, geom, *, cin, cout, tmode=L.VT_TPAD_ZERO, bias=True):
    g = dy.float()[..., :cout].permute(0, 4, 1, 2, 3)
    dw = torch.nn.grad.conv3d_weight(_virtual(x, geom, tmode, cin), (cout, cin, geom.kt, geom.kh, geom.kw), g, stride=(geom.st, geom.sh, geom.sw))
    return dw, (g.sum(dim=(0, 2, 3, 4)) if bias else None)


def conv_dgrad(dy, w, geom, *, cin, cout, tmode=L.VT_TPAD_ZERO, acc=None, dx_dtype=None):
    """gradient of the virtual input (torch's own convolution backward), then the adjoint of S.virtual_input: pads cropped, replicated
    front frames summed into frame 0, up-sampled positions summed into their source"""
    dx_dtype = dx_dtype or dy.dtype
    B, To, Ho, Wo, lddy = dy.shape
    Tv, Hv, Wv = To - geom.pt - geom.pt_hi + geom.kt - 1, Ho - geom.ph - geom.ph_hi + geom.kh - 1, Wo - geom.pw - geom.pw_hi + geom.kw - 1
    w5 = w.float().reshape(cin, geom.kt, geom.kh, geom.kw, lddy)[..., :cout].permute(4, 0, 1, 2, 3).flip(2, 3, 4).contiguous()
    full = (B, cin, geom.pt + Tv + geom.pt_hi, geom.ph + Hv + geom.ph_hi, geom.pw + Wv + geom.pw_hi)
    gv = torch.nn.grad.conv3d_input(full, w5, dy.float()[..., :cout].permute(0, 4, 1, 2, 3))
    gv = gv[:, :, :geom.pt + Tv, geom.ph:geom.ph + Hv, geom.pw:geom.pw + Wv].permute(0, 2, 3, 4, 1)
    rep = geom.pt if tmode == L.VT_TPAD_REPLICATE else 0
    dx = grad_fold(gv[:, geom.pt - rep:], ups_t=geom.ups_t, ups_s=geom.ups_s, rep=rep)
    dx = F.pad(dx, (0, pad_channels(cin) - cin))
    if acc is not None:
        dx = dx + acc.float()
    return dx.to(dx_dtype)


def layernorm_act_backward(y, dn, gamma, beta, *, silu, eps=1e-6, c=None, dx_dtype=None):
    c = c or y.shape[-1]
    x, g = y.float()[..., :c], dn.float()[..., :c]
    rstd = (x.var(dim=-1, unbiased=False, keepdim=True) + eps).rsqrt()
    xh = (x - x.mean(dim=-1, keepdim=True)) * rstd
    if silu:
        n = xh * gamma + beta
        sg = torch.sigmoid(n)
        g = g * (sg * (1 + n * (1 - sg)))
    red = tuple(range(x.dim() - 1))
    dxh = g * gamma
    dx = rstd * (dxh - dxh.mean(dim=-1, keepdim=True) - xh * (dxh * xh).mean(dim=-1, keepdim=True))
    return F.pad(dx, (0, y.shape[-1] - c)).to(dx_dtype or y.dtype), (g * xh).sum(dim=red), g.sum(dim=red)


def grad_fold(src, *, ups_t=0, ups_s=0, rep=0, c=None, acc=None, out_dtype=None):
    d = src.float()
    if rep:
        d = torch.cat([d[:, :rep + 1].sum(dim=1, keepdim=True), d[:, rep + 1:]], dim=1)
    if ups_t:
        d = d[:, 0::2] + d[:, 1::2]
    if ups_s:
        d = (d[:, :, 0::2, 0::2] + d[:, :, 0::2, 1::2]) + (d[:, :, 1::2, 0::2] + d[:, :, 1::2, 1::2])
    if acc is not None:
        d = d + acc.float()
    return d.to(out_dtype or src.dtype).contiguous()


def softmax_rows_backward(p, dp, scale, cols=None, ld_out=None):
    cols = cols or dp.shape[-1]
    pf = p.float()[..., :cols]
    ds = scale * pf * (dp - (pf * dp).sum(dim=-1, keepdim=True))
    return F.pad(ds, (0, (ld_out or p.shape[-1]) - cols)).to(p.dtype).contiguous()


def transpose_batched(x, rows=None, cols=None, ld_out=None):
    Z, Rr, ld = x.shape
    cols = cols or ld
    return F.pad(x[:, :, :cols].transpose(1, 2), (0, (ld_out or pad_channels(Rr)) - Rr)).contiguous()


def upsample_mix(u, c, mix_factor, ch=None):
    ch = ch or u.shape[-1]
    a = torch.sigmoid(mix_factor.float())
    y = torch.zeros_like(u)
    y[..., :ch] = (a * u.float()[..., :ch] + (1 - a) * c.float()[..., :ch]).to(u.dtype)
    return y


def upsample_mix_backward(dy, u, c, mix_factor, ch=None):
    ch = ch or dy.shape[-1]
    a = torch.sigmoid(mix_factor.float())
    g = F.pad(dy.float()[..., :ch], (0, dy.shape[-1] - ch))
    dmix = a * (1 - a) * (g * (u.float() - c.float())).sum().reshape(1)
    return (a * g).to(dy.dtype), ((1 - a) * g).to(dy.dtype), dmix


def time_lerp2x_backward(dy, t0, n, out, out_t0):
    """adjoint of the x2 linear interpolation in time (half-pixel centres, clamped at both ends) of n frames on their own"""
    dx = torch.zeros((dy.shape[0], n) + tuple(dy.shape[2:]))
    for j in range(2 * n):
        src = max((j + 0.5) * 0.5 - 0.5, 0.0)
        a = int(src)
        b = a + (1 if a < n - 1 else 0)
        dx[:, a] += (1 - (src - a)) * dy[:, t0 + j].float()
        dx[:, b] += (src - a) * dy[:, t0 + j].float()
    out[:, out_t0:out_t0 + n] = dx.to(out.dtype)
    return out


def grad_ncthw_to_ndhwc(g, dtype, tpad=0, ld=None):
    B, Cc, T, H, W = g.shape
    y = torch.zeros((B, T + tpad, H, W, ld or pad_channels(Cc)), dtype=dtype)
    y[:, tpad:, ..., :Cc] = g.permute(0, 2, 3, 4, 1).to(dtype)
    return y


def grad_add(a, b):
    return (a.float() + b.float()).to(a.dtype)


ALL = ["pack_conv_weight_dgrad", "conv_wgrad", "conv_dgrad", "layernorm_act_backward", "grad_fold", "softmax_rows_backward", "transpose_batched",
       "upsample_mix", "upsample_mix_backward", "time_lerp2x_backward", "grad_ncthw_to_ndhwc", "grad_add"]


@contextlib.contextmanager
def patched_ops():
    """vidtok_amd.ops with the torch statements of the forward (torch_ops_ref) and of the backward (this file) swapped in; yields a dict
    that counts the calls of every swapped operator"""
    import vidtok_amd.ops as ops

    calls = {}

    def counted(name, fn):
        def inner(*a, **kw):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a, **kw)
        return inner

    with pytest.MonkeyPatch.context() as mp:
        for mod, names in ((R, R.ALL), (globals(), ALL)):
            for name in names:
                fn = mod[name] if isinstance(mod, dict) else getattr(mod, name)
                mp.setattr(ops, name, counted(name, fn))
        yield calls
