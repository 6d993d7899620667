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

`recompute=` trades tape for arithmetic (activation recomputation).  "none" keeps everything listed above.  "norms" drops the output
of every LayerNorm(+SiLU) and rebuilds it from the saved pre-norm rows right before the weight gradient that reads it.  "stages" keeps
only the latent rows, the input of every stage and the tensor in front of norm_out; the backward re-runs one stage's forward at a time.
Both rebuild with the forward's launches on the forward's operands in the tape's dtype, so every result has the bits of "none"; a
decoder parameter changed in place between forward and backward would be repacked and silently change them, so that is an error.

A whole clip only (first-chunk form: zero pad for v1.0, first-frame replicate for v1.1; the chunk caches are neither read nor
written), `norm_type: layernorm`, compute dtype fp32 or bf16.
"""
import typing

import torch

from . import lib as L
from . import modules as M
from . import ops
from .ops import ConvGeom
from . import packing
from .packing import ConvSite

RECOMPUTE_MODES = ("none", "norms", "stages")


def check_recompute(recompute):
    if recompute not in RECOMPUTE_MODES:
        raise ValueError(f"decode_with_grad: recompute={recompute!r}: one of {RECOMPUTE_MODES}")


def _wants(p):
    return p is not None and p.requires_grad


def _reads_input(s: ConvSite):
    """does the backward of this convolution read its input (vt_conv_wgrad does; vt_conv_dgrad reads the weight only)"""
    return _wants(s.conv.weight) or _wants(s.conv.bias)


def _conv_backward(s: ConvSite, x, dy, grads, acc=None, need_dx=True):
    """parameter gradients of one convolution into `grads`; returns dx (+ acc), or None when nobody asks for it"""
    if _reads_input(s):
        dw, db = ops.conv_wgrad(x, dy, s.geom, cin=s.cin, cout=s.cout, tmode=s.clip_tmode, bias=s.conv.bias is not None)
        grads[s.conv.weight] = dw.view(s.conv.weight.shape)
        if s.conv.bias is not None:
            grads[s.conv.bias] = db
    if not need_dx:
        return None
    return s.dgrad(dy, acc=acc)


def _norm(norm, x, silu, dt):
    g, b = norm.affine()
    return ops.layernorm_act(x, g, b, silu=silu, eps=norm.norm.eps, out_dtype=dt, c=norm.norm.normalized_shape[0])


def _norm_backward(norm, y, dn, silu, grads):
    g, b = norm.affine()
    dx, dg, db = ops.layernorm_act_backward(y, dn, g, b, silu=silu, eps=norm.norm.eps, c=norm.norm.normalized_shape[0])
    grads[norm.norm.weight], grads[norm.norm.bias] = dg, db
    return dx


# ---- stages: forward(x, dt) -> (y, saved), backward(saved, dy, grads, dt) -> dx; lean(saved) = saved without what recompute="norms"
# rebuilds (a None in the place of a LayerNorm output: backward runs the forward's _norm call again, in the tape's dt) -----------------
class _Stage:
    def lean(self, saved):
        return saved


class _ResStage(_Stage):
    """ResnetBlock / ResnetCausalBlock / ResnetCausalBlock1D: LN-SiLU-conv LN-SiLU-conv (+ shortcut conv) + x"""

    def __init__(self, blk):
        self.blk = blk
        self.c1, self.c2, self.nin = blk.sites

    def forward(self, x, dt):
        h1 = _norm(self.blk.norm1, x, True, dt)
        c1 = self.c1.run_clip(h1, dt)
        h2 = _norm(self.blk.norm2, c1, True, dt)
        sc = x if self.nin is None else self.nin.run_clip(x, dt)
        return self.c2.run_clip(h2, dt, res=sc, res_mode=L.VT_RES_ADD), (x, h1, c1, h2)

    def lean(self, saved):
        x, _h1, c1, _h2 = saved
        return (x, None, c1, None)

    def backward(self, saved, dy, grads, dt):
        x, h1, c1, h2 = saved
        if h2 is None and _reads_input(self.c2):
            h2 = _norm(self.blk.norm2, c1, True, dt)
        dh2 = _conv_backward(self.c2, h2, dy, grads)
        del h2
        dc1 = _norm_backward(self.blk.norm2, c1, dh2, True, grads)
        if h1 is None and _reads_input(self.c1):
            h1 = _norm(self.blk.norm1, x, True, dt)
        dh1 = _conv_backward(self.c1, h1, dc1, grads)
        del h1
        dx = _norm_backward(self.blk.norm1, x, dh1, True, grads)
        if self.nin is None:
            return ops.grad_add(dx, dy)
        return _conv_backward(self.nin, x, dy, grads, acc=dx)


class _AttnStage(_Stage):
    """AttnBlockWrapper: LN, q / k / v 1x1x1, softmax(q k^T / sqrt(C)) v per frame, proj_out, + x"""

    def __init__(self, blk):
        self.blk = blk
        self.q, self.k, self.v, self.proj = blk.q.site, blk.k.site, blk.v.site, blk.proj_out.site

    def forward(self, x, dt):
        B, T, H, W, Cc = x.shape
        assert Cc == self.blk.in_channels, "attention channels must be a multiple of 8"
        S, Z = H * W, B * T
        Sp = ops.pad_channels(S)
        hn = _norm(self.blk.norm, x, False, dt)
        q, k, v = (s.run_clip(hn, dt).view(Z, S, Cc) for s in (self.q, self.k, self.v))
        s = ops.gemm_nt(q, k, out_dtype=torch.float32)                               # [Z, S, S]
        p = ops.softmax_rows(s, float(Cc) ** -0.5, dt, ld_out=Sp)                     # [Z, S, Sp]
        o = ops.gemm_nt(p, ops.transpose_batched(v, ld_out=Sp)).view(B, T, H, W, Cc)
        return self.proj.run_clip(o, dt, res=x, res_mode=L.VT_RES_ADD), (x, hn, q, k, v, p, o)

    def lean(self, saved):
        return (saved[0], None) + tuple(saved[2:])

    def backward(self, saved, dy, grads, dt):
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
        if hn is None and any(_reads_input(s) for s in (self.q, self.k, self.v)):
            hn = _norm(self.blk.norm, x, False, dt)
        dhn = None
        for s, g in ((self.q, dq), (self.k, dk), (self.v, dv)):
            dhn = _conv_backward(s, hn, g.view(B, T, H, W, Cc), grads, acc=dhn)
        del hn
        return ops.grad_add(_norm_backward(self.blk.norm, x, dhn, False, grads), dy)


class _SpaceUpStage(_Stage):
    """Upsample: nearest x2 + conv3x3 as ONE convolution whose gather folds the up-sampling (the view tests/backward_sites.py takes)"""

    def __init__(self, up):
        if not up.with_conv:
            raise NotImplementedError("decode_with_grad: Upsample(with_conv=False) has no backward here")
        self.s = up.fold_site

    def forward(self, x, dt):
        return self.s.run_clip(x, dt), (x,)

    def backward(self, saved, dy, grads, dt):
        return _conv_backward(self.s, saved[0], dy, grads)


class _TimeUpStage(_Stage):
    """TimeUpsampleResCausal2x on a whole clip: u = up(x) (nearest, or the v1.1 first-chunk trilinear head / tail split), y = a u + (1 - a) conv(u)"""

    def __init__(self, up):
        self.up = up
        self.s = up.conv.site
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
        c = self.s.run_clip(u, dt)
        return ops.upsample_mix(u, c, self.up.mix_factor.detach(), ch=self.s.cout), (u, c, x.shape)

    def backward(self, saved, dy, grads, dt):
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


class Tape(typing.NamedTuple):
    """what train_forward leaves for train_backward"""
    stages: list
    saved: list                    # per stage: its saved tuple ("none"), the tuple without LayerNorm outputs ("norms"), its input ("stages")
    cin: ConvSite
    cout: ConvSite
    h0: torch.Tensor               # the latent rows
    h: torch.Tensor                # the tensor in front of norm_out
    hn: typing.Optional[torch.Tensor]     # norm_out's output; None when the backward rebuilds it
    trim: int
    dt: torch.dtype
    recompute: str
    versions: typing.Optional[list]       # [(name, p._version)] of every decoder parameter at forward time; None for "none"
    arith: typing.Optional[str]           # PackedCache.arith the forward packed its weights with


def train_forward(dec, z, recompute="none"):
    """the recording pass: (x_hat NCTHW fp32, tape)"""
    check_recompute(recompute)
    dt = dec.compute_dtype
    stages = [_stage(m) for m in dec.train_stage_modules()]
    cin, cout = dec.conv_in.site, dec.conv_out.site
    h0 = ops.ncthw_to_ndhwc(z.detach().contiguous().float(), dt)
    h = cin.run_clip(h0, dt)
    saved = []
    for st in stages:
        if recompute == "stages":
            saved.append(h)                         # the stage's input alone: the backward runs st.forward again
            h = st.forward(h, dt)[0]
            continue
        h, keep = st.forward(h, dt)
        saved.append(keep if recompute == "none" else st.lean(keep))
    hn = _norm(dec.norm_out, h, True, dt)
    trim = dec.time_padding if dec.version == "v1_0" else 0
    y = cout.run_clip(hn, dt, out_layout=L.VT_NCTHW, t_trim=trim)
    if recompute == "none":
        return y, Tape(stages, saved, cin, cout, h0, h, hn, trim, dt, recompute, None, None)
    # what a recomputation must find unchanged: every parameter (the packed-weight caches repack on a new version) and the weight arithmetic
    versions = [(n, p._version) for n, p in dec.named_parameters()]
    return y, Tape(stages, saved, cin, cout, h0, h, None, trim, dt, recompute, versions, cin.pack.arith)


def tape_tensors(tape):
    """the distinct tensors a tape holds between forward and backward (tensors that share storage once)"""
    seen, out = set(), []

    def visit(v):
        if isinstance(v, torch.Tensor):
            key = v.untyped_storage().data_ptr() or id(v)          # empty tensors all report address 0: each is its own
            if key not in seen:
                seen.add(key)
                out.append(v)
        elif isinstance(v, (tuple, list)) and not isinstance(v, torch.Size):
            for e in v:
                visit(e)

    visit(tape.saved)
    visit((tape.h0, tape.h, tape.hn))
    return out


def tape_bytes(tape):
    """bytes of activations a tape keeps alive: numel * element_size over tape_tensors(tape)"""
    return sum(t.numel() * t.element_size() for t in tape_tensors(tape))


def _check_unchanged(dec, versions):
    for (name, ver), (_n, p) in zip(versions, dec.named_parameters()):
        if p._version != ver:
            raise RuntimeError(f"decode_with_grad: decoder parameter {name!r} was modified in place between the forward and this backward "
                               f"(version {ver} -> {p._version}): the recomputation would run with the new weights. Call backward() before "
                               f"optimizer.step(), or use recompute=\"none\"")


class _tape_arith:
    """the packed-weight arithmetic of the forward for the duration of a recomputing backward (set_compute_dtype may have moved on: a
    forward is only accepted in fp32 / bf16, arith None, but "bf16x3" may be chosen before the backward runs).  packing.set_arith gives
    every non-pinned cache under a module the same arithmetic, so conv_in's cache (`probe`) speaks for all of them, here and on exit"""

    def __init__(self, dec, arith, probe):
        self.dec, self.arith, self.was = dec, arith, probe.arith

    def __enter__(self):
        if self.was != self.arith:
            packing.set_arith(self.dec, self.arith)

    def __exit__(self, *exc):
        if self.was != self.arith:
            packing.set_arith(self.dec, self.was)


def train_backward(dec, tape, cot, need_dz):
    """({parameter: gradient fp32 in the parameter's layout}, dz NCTHW fp32 or None) for the cotangent of train_forward's result"""
    *_, recompute, versions, arith = tape          # (a tape already used up is None: a second backward fails here, as it always has)
    if recompute == "none":
        return _backward(dec, tape, cot, need_dz)
    _check_unchanged(dec, versions)
    with _tape_arith(dec, arith, tape.cin.pack):
        return _backward(dec, tape, cot, need_dz)


def _backward(dec, tape, cot, need_dz):
    stages, saved, cin, cout, h0, h, hn, trim, dt, recompute, _versions, _arith = tape
    grads = {}
    dy = ops.grad_ncthw_to_ndhwc(cot.contiguous().float(), dt, tpad=trim, ld=ops.pad_channels(cout.cout))
    if hn is None and _reads_input(cout):
        hn = _norm(dec.norm_out, h, True, dt)
    d = _conv_backward(cout, hn, dy, grads)
    del hn
    if dt != torch.float32 and _wants(cout.conv.bias):
        # conv_out's bias gradient is the plain sum of the cotangent: taken from the fp32 cotangent, not from its 16-bit rounding (the sum of
        # ~10^6 rounding errors is 1e-3 of a sum that partly cancels) -- vt_conv_wgrad of a 1x1x1 site on the fp32 rows, its db alone
        dy32 = ops.grad_ncthw_to_ndhwc(cot.contiguous().float(), torch.float32, tpad=trim, ld=dy.shape[-1])
        grads[cout.conv.bias] = ops.conv_wgrad(dy32, dy32, ConvGeom(), cin=cout.cout, cout=cout.cout)[1]
    d = _norm_backward(dec.norm_out, h, d, True, grads)
    for i in reversed(range(len(stages))):
        keep = saved[i]
        if recompute == "stages":
            keep = stages[i].forward(keep, dt)[1]           # the stage's saved tuple again, from its input; its output is dropped here
        d = stages[i].backward(keep, d, grads, dt)
        if recompute != "none":
            saved[i] = keep = None                          # the tape is used up as the walk goes
    dz = _conv_backward(cin, h0, d, grads, need_dx=need_dz)
    return grads, (ops.ndhwc_to_ncthw(dz, cin.cin) if need_dz else None)


class DecodeFunction(torch.autograd.Function):
    """decoder.forward_train(z) as one autograd node: inputs (z, every decoder parameter), output x_hat"""

    @staticmethod
    def forward(ctx, dec, z, recompute, *params):
        y, tape = train_forward(dec, z, recompute)
        ctx.dec, ctx.tape, ctx.params = dec, tape, params
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, cot):
        grads, dz = train_backward(ctx.dec, ctx.tape, cot, ctx.needs_input_grad[1])
        ctx.tape = None
        out = []
        for i, p in enumerate(ctx.params):
            g = grads.get(p) if ctx.needs_input_grad[3 + i] else None
            if ctx.needs_input_grad[3 + i] and g is None:
                raise RuntimeError("decode_with_grad: a decoder parameter received no gradient")
            out.append(None if g is None else g.view(p.shape))
        return (None, dz, None) + tuple(out)


def forward_train(dec, z, recompute="none"):
    check_recompute(recompute)
    check_supported(dec)
    if not (isinstance(z, torch.Tensor) and z.dim() == 5 and z.dtype == torch.float32):
        raise TypeError("decode_with_grad: z must be an fp32 [B, D, T', H', W'] tensor")
    return DecodeFunction.apply(dec, z, recompute, *dec.parameters())
