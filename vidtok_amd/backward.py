"""Differentiable decode of the causal decoders: a recording forward and its backward, both on the HIP kernels.

`DecoderCausal3DPadding.forward_train(z)` (reached through `AutoencodingEngine.decode_with_grad`) returns what `decode(z)` returns,
attached to the autograd graph by ONE `torch.autograd.Function`.  The forward is a recording pass built from the ops of the
inference path, un-fused wherever the backward needs a tensor the fused form never writes: every convolution runs without `ln=`
and is followed by `ops.layernorm_act`, the temporal blocks run as two convolutions, the attention as GEMM - softmax - GEMM, the
time up-samplers as up-sampling + convolution + `ops.upsample_mix`, the spatial up-sampler as one 3 x 3 convolution with the
nearest x2 folded into its gather.  Each stage keeps what its backward reads:

  convolution          its input (vt_conv_wgrad needs it; vt_conv_dgrad needs the weight only)
  LayerNorm(+SiLU)     the pre-norm rows (mean / rstd are recomputed)
  attention            q, k, v, the probabilities P and the context o
  time up-sampler      the up-sampled tensor u and conv(u)

The backward walks the stages in reverse.  Data gradients: `ops.conv_dgrad` (the forward implicit-GEMM tiles over dy with the
transposed, tap-flipped weight; `acc=` adds the gradient already held at a junction); parameter gradients: `ops.conv_wgrad`,
`ops.layernorm_act_backward`, `ops.upsample_mix_backward`.  Nothing uses float atomics: two runs give the same bits.

A whole clip only (first-chunk form: zero pad for v1.0, first-frame replicate for v1.1; the chunk caches are neither read nor
written), `norm_type: layernorm`, compute dtype fp32 or bf16.
"""
import dataclasses

import torch

from . import lib as L
from . import modules as M
from . import ops
from .ops import ConvGeom
from .packing import DgradPackCache, PackedCache


@dataclasses.dataclass
class _Site:
    """one convolution of the decoder as the kernels see it"""
    conv: torch.nn.Module          # nn.Conv1d / Conv2d / Conv3d parameter holder
    pack: PackedCache
    geom: ConvGeom
    tmode: int
    cin: int
    cout: int

    def dpack(self):
        return self.conv.__dict__.setdefault("_dgrad_pack", DgradPackCache())


def _site(mod, pack=None, geom=None):
    if isinstance(mod, (M.CausalConv3d, M.CausalConv1d)):
        tmode = L.VT_TPAD_ZERO if (mod.version == "v1_0" or mod.time_pad == 0) else L.VT_TPAD_REPLICATE
        g = mod.geom(0) if isinstance(mod, M.CausalConv3d) else ConvGeom(kt=mod.k, st=mod.stride, pt=mod.time_pad)
        return _Site(mod.conv, mod._pack, g, tmode, mod.conv.in_channels, mod.chan_out)
    return _Site(mod, pack, geom, L.VT_TPAD_ZERO, mod.in_channels, mod.out_channels)


def _conv(s: _Site, x, dt, **kw):
    w, b = s.pack.get(s.conv.weight, s.conv.bias, dt, cin_stored=x.shape[-1])
    return ops.conv(x, w, b, s.geom, cout=s.cout, tmode=s.tmode, **kw)


def _wants(p):
    return p is not None and p.requires_grad


def _conv_backward(s: _Site, x, dy, grads, acc=None, need_dx=True):
    """parameter gradients of one convolution into `grads`; returns dx (+ acc), or None when nobody asks for it"""
    if _wants(s.conv.weight) or _wants(s.conv.bias):
        dw, db = ops.conv_wgrad(x, dy, s.geom, cin=s.cin, cout=s.cout, tmode=s.tmode, bias=s.conv.bias is not None)
        grads[s.conv.weight] = dw.view(s.conv.weight.shape)
        if s.conv.bias is not None:
            grads[s.conv.bias] = db
    if not need_dx:
        return None
    wt = s.dpack().get(s.conv.weight, dy.dtype, dy.shape[-1])
    return ops.conv_dgrad(dy, wt, s.geom, cin=s.cin, cout=s.cout, tmode=s.tmode, acc=acc)


def _norm(norm, x, silu, dt):
    g, b = norm.affine()
    return ops.layernorm_act(x, g, b, silu=silu, eps=norm.norm.eps, out_dtype=dt, c=norm.norm.normalized_shape[0])


def _norm_backward(norm, y, dn, silu, grads):
    g, b = norm.affine()
    dx, dg, db = ops.layernorm_act_backward(y, dn, g, b, silu=silu, eps=norm.norm.eps, c=norm.norm.normalized_shape[0])
    grads[norm.norm.weight], grads[norm.norm.bias] = dg, db
    return dx


# ---- stages: forward(x) -> (y, saved), backward(saved, dy, grads) -> dx ------------------------------------------------------
class _ResStage:
    """ResnetBlock / ResnetCausalBlock / ResnetCausalBlock1D: LN-SiLU-conv LN-SiLU-conv (+ shortcut conv) + x"""

    def __init__(self, blk):
        self.blk = blk
        if isinstance(blk, M.ResnetBlock):
            self.c1, self.c2 = _site(blk.conv1, blk._p1, M._G3x3), _site(blk.conv2, blk._p2, M._G3x3)
            self.nin = _site(blk.nin_shortcut, blk._p3, M._G1x1) if blk.in_channels != blk.out_channels else None
        else:
            self.c1, self.c2 = _site(blk.conv1), _site(blk.conv2)
            self.nin = _site(blk.nin_shortcut) if blk.in_channels != blk.out_channels else None

    def forward(self, x, dt):
        h1 = _norm(self.blk.norm1, x, True, dt)
        c1 = _conv(self.c1, h1, dt)
        h2 = _norm(self.blk.norm2, c1, True, dt)
        sc = x if self.nin is None else _conv(self.nin, x, dt)
        return _conv(self.c2, h2, dt, res=sc, res_mode=L.VT_RES_ADD), (x, h1, c1, h2)

    def backward(self, saved, dy, grads):
        x, h1, c1, h2 = saved
        dh2 = _conv_backward(self.c2, h2, dy, grads)
        dc1 = _norm_backward(self.blk.norm2, c1, dh2, True, grads)
        dh1 = _conv_backward(self.c1, h1, dc1, grads)
        dx = _norm_backward(self.blk.norm1, x, dh1, True, grads)
        if self.nin is None:
            return ops.grad_add(dx, dy)
        return _conv_backward(self.nin, x, dy, grads, acc=dx)


class _AttnStage:
    """AttnBlockWrapper: LN, q / k / v 1x1x1, softmax(q k^T / sqrt(C)) v per frame, proj_out, + x"""

    def __init__(self, blk):
        self.blk = blk
        self.q, self.k, self.v, self.proj = _site(blk.q), _site(blk.k), _site(blk.v), _site(blk.proj_out)

    def forward(self, x, dt):
        B, T, H, W, Cc = x.shape
        assert Cc == self.blk.in_channels, "attention channels must be a multiple of 8"
        S, Z = H * W, B * T
        Sp = ops.pad_channels(S)
        hn = _norm(self.blk.norm, x, False, dt)
        q, k, v = (_conv(s, hn, dt).view(Z, S, Cc) for s in (self.q, self.k, self.v))
        s = ops.gemm_nt(q, k, out_dtype=torch.float32)                               # [Z, S, S]
        p = ops.softmax_rows(s, float(Cc) ** -0.5, dt, ld_out=Sp)                     # [Z, S, Sp]
        o = ops.gemm_nt(p, ops.transpose_batched(v, ld_out=Sp)).view(B, T, H, W, Cc)
        return _conv(self.proj, o, dt, res=x, res_mode=L.VT_RES_ADD), (x, hn, q, k, v, p, o)

    def backward(self, saved, dy, grads):
        x, hn, q, k, v, p, o = saved
        B, T, H, W, Cc = x.shape
        Z, S = q.shape[:2]
        Sp = p.shape[-1]
        do = _conv_backward(self.proj, o, dy, grads).view(Z, S, Cc)
        dp = ops.gemm_nt(do, v, out_dtype=torch.float32)                                                        # dP = dO V^T
        dv = ops.gemm_nt(ops.transpose_batched(p, cols=S, ld_out=Sp), ops.transpose_batched(do, ld_out=Sp))      # dV = P^T dO
        ds = ops.softmax_rows_backward(p, dp, float(Cc) ** -0.5, cols=S, ld_out=Sp)
        dq = ops.gemm_nt(ds, ops.transpose_batched(k, ld_out=Sp))                                                # dQ = dS K
        dk = ops.gemm_nt(ops.transpose_batched(ds, cols=S, ld_out=Sp), ops.transpose_batched(q, ld_out=Sp))      # dK = dS^T Q
        dhn = None
        for s, g in ((self.q, dq), (self.k, dk), (self.v, dv)):
            dhn = _conv_backward(s, hn, g.view(B, T, H, W, Cc), grads, acc=dhn)
        return ops.grad_add(_norm_backward(self.blk.norm, x, dhn, False, grads), dy)


class _SpaceUpStage:
    """Upsample: nearest x2 + conv3x3 as ONE convolution whose gather folds the up-sampling (the view tests/backward_sites.py takes)"""

    def __init__(self, up):
        if not up.with_conv:
            raise NotImplementedError("decode_with_grad: Upsample(with_conv=False) has no backward here")
        pack = up.__dict__.setdefault("_train_pack", PackedCache())
        self.s = _site(up.conv, pack, dataclasses.replace(M._G3x3, ups_s=1))

    def forward(self, x, dt):
        return _conv(self.s, x, dt), (x,)

    def backward(self, saved, dy, grads):
        return _conv_backward(self.s, saved[0], dy, grads)


class _TimeUpStage:
    """TimeUpsampleResCausal2x on a whole clip: u = up(x) (nearest, or the v1.1 first-chunk trilinear head / tail split), y = a u + (1 - a) conv(u)"""

    def __init__(self, up):
        self.up = up
        self.s = _site(up.conv)
        self.trilinear = up.version == "v1_1" and up.enable_cached

    def _spans(self, T):
        """[(first source frame, frames)] that are interpolated on their own (modules.py::_interp_v11, first chunk)"""
        n = self.up.num_temp_upsample
        hn = min(n, T)
        return [(0, hn)] + ([(n, T - n)] if T > n else [])

    def forward(self, x, dt):
        T = x.shape[1]
        if self.trilinear:
            u = torch.empty((x.shape[0], 2 * T) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device)
            for t0, n in self._spans(T):
                ops.time_lerp2x(ops.gather_frames(x, list(range(t0, t0 + n))), out=u, out_t0=2 * t0)
        else:
            u = ops.gather_frames(x, [t // 2 for t in range(2 * T)])
        c = _conv(self.s, u, dt)
        return ops.upsample_mix(u, c, self.up.mix_factor.detach(), ch=self.s.cout), (u, c, x.shape)

    def backward(self, saved, dy, grads):
        u, c, xshape = saved
        du, dc, dmix = ops.upsample_mix_backward(dy, u, c, self.up.mix_factor.detach(), ch=self.s.cout)
        grads[self.up.mix_factor] = dmix
        du = _conv_backward(self.s, u, dc, grads, acc=du)
        if not self.trilinear:
            return ops.grad_fold(du, ups_t=1, c=self.s.cin)
        dx = torch.empty(tuple(xshape), dtype=du.dtype, device=du.device)
        for t0, n in self._spans(xshape[1]):
            ops.time_lerp2x_backward(du, 2 * t0, n, dx, t0)
        return dx


def _stage(m):
    if isinstance(m, (M.ResnetBlock, M.ResnetCausalBlock, M.ResnetCausalBlock1D)):
        return _ResStage(m)
    if isinstance(m, M.AttnBlockWrapper):
        return _AttnStage(m)
    if isinstance(m, M.Upsample):
        return _SpaceUpStage(m)
    if isinstance(m, M.TimeUpsampleResCausal2x):
        return _TimeUpStage(m)
    raise NotImplementedError(f"decode_with_grad: no backward for {type(m).__name__}")


def check_supported(dec):
    """raise NotImplementedError for what the training path does not cover (silently wrong gradients are the failure to avoid)"""
    if dec.norm_type != "layernorm":
        raise NotImplementedError(f"decode_with_grad: norm_type={dec.norm_type!r}: only the LayerNorm decoders have a backward (vt_layernorm_act_backward)")
    if dec.give_pre_end or dec.tanh_out:
        raise NotImplementedError("decode_with_grad: give_pre_end / tanh_out decoders have no backward")
    if dec.compute_dtype not in (torch.float32, torch.bfloat16):
        raise NotImplementedError(f"decode_with_grad: compute dtype {dec.compute_dtype}: the backward kernels take fp32 or bf16 (fp16 has no loss scaling here)")


def train_forward(dec, z):
    """the recording pass: (x_hat NCTHW fp32, tape)"""
    dt = dec.compute_dtype
    stages = [_stage(m) for m in dec.train_stage_modules()]
    cin, cout = _site(dec.conv_in), _site(dec.conv_out)
    h0 = ops.ncthw_to_ndhwc(z.detach().contiguous().float(), dt)
    h = _conv(cin, h0, dt)
    saved = []
    for st in stages:
        h, keep = st.forward(h, dt)
        saved.append(keep)
    hn = _norm(dec.norm_out, h, True, dt)
    trim = dec.time_padding if dec.version == "v1_0" else 0
    y = _conv(cout, hn, dt, out_layout=L.VT_NCTHW, t_trim=trim)
    return y, (stages, saved, cin, cout, h0, h, hn, trim, dt)


def train_backward(dec, tape, cot, need_dz):
    """({parameter: gradient fp32 in the parameter's layout}, dz NCTHW fp32 or None) for the cotangent of train_forward's result"""
    stages, saved, cin, cout, h0, h, hn, trim, dt = tape
    grads = {}
    dy = ops.grad_ncthw_to_ndhwc(cot.contiguous().float(), dt, tpad=trim, ld=ops.pad_channels(cout.cout))
    d = _conv_backward(cout, hn, dy, grads)
    if dt != torch.float32 and _wants(cout.conv.bias):
        # conv_out's bias gradient is the plain sum of the cotangent: taken from the fp32 cotangent, not from its 16-bit rounding (the sum of
        # ~10^6 rounding errors is 1e-3 of a sum that partly cancels) -- vt_conv_wgrad of a 1x1x1 site on the fp32 rows, its db alone
        dy32 = ops.grad_ncthw_to_ndhwc(cot.contiguous().float(), torch.float32, tpad=trim, ld=dy.shape[-1])
        grads[cout.conv.bias] = ops.conv_wgrad(dy32, dy32, ConvGeom(), cin=cout.cout, cout=cout.cout)[1]
    d = _norm_backward(dec.norm_out, h, d, True, grads)
    for st, keep in zip(reversed(stages), reversed(saved)):
        d = st.backward(keep, d, grads)
    dz = _conv_backward(cin, h0, d, grads, need_dx=need_dz)
    return grads, (ops.ndhwc_to_ncthw(dz, cin.cin) if need_dz else None)


class DecodeFunction(torch.autograd.Function):
    """decoder.forward_train(z) as one autograd node: inputs (z, every decoder parameter), output x_hat"""

    @staticmethod
    def forward(ctx, dec, z, *params):
        y, tape = train_forward(dec, z)
        ctx.dec, ctx.tape, ctx.params = dec, tape, params
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, cot):
        grads, dz = train_backward(ctx.dec, ctx.tape, cot, ctx.needs_input_grad[1])
        ctx.tape = None
        out = []
        for i, p in enumerate(ctx.params):
            g = grads.get(p) if ctx.needs_input_grad[2 + i] else None
            if ctx.needs_input_grad[2 + i] and g is None:
                raise RuntimeError("decode_with_grad: a decoder parameter received no gradient")
            out.append(None if g is None else g.view(p.shape))
        return (None, dz) + tuple(out)


def forward_train(dec, z):
    check_supported(dec)
    if not (isinstance(z, torch.Tensor) and z.dim() == 5 and z.dtype == torch.float32):
        raise TypeError("decode_with_grad: z must be an fp32 [B, D, T', H', W'] tensor")
    return DecodeFunction.apply(dec, z, *dec.parameters())
