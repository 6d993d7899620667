"""The 2-D PatchGAN discriminator of the reference's adversarial loss on the HIP kernels.

`NLayerDiscriminator` mirrors `vidtok.modules.discriminator.NLayerDiscriminator` (reference discriminator.py:88-137, the network of
`GeneralLPIPSWithDiscriminator` with `disc_type: 2d`, losses.py:187-249): the same constructor arguments, the same `main.*` state_dict
keys and shapes (a reference state_dict loads with strict=True), `forward(x) -> logits` on NCHW frames.  The submodules of `main` hold
the parameters and are never called: every convolution is a vt_conv launch on NDHWC activations with one frame, BatchNorm + LeakyReLU
is vt_batchnorm_stats + vt_batchnorm_act (include/vidtok_amd.h, "PatchGAN discriminator").  Arithmetic: fp32 by default,
`set_compute_dtype(torch.bfloat16)` or the dtype of the caller's torch.autocast("cuda") region; statistics and epilogues are fp32 in
both.  `self.training` selects batch statistics (running statistics updated as nn.BatchNorm2d does) or the running statistics.

`forward_with_grad` is the same pass as one autograd node with a HIP backward: the gradient with respect to the frames (the generator
step, frames from `decode_with_grad`) and to every parameter that requires grad (the discriminator step).  The loss formulas on the
logits stay torch statements of the caller ("Adversarial term").
"""
import torch
import torch.nn as nn

from . import lib as L
from . import ops
from .packing import ConvSite

SLOPE = 0.2
_MODES = (torch.float32, torch.bfloat16)
_FP16_MSG = "compute dtype torch.float16: the backward kernels take float32 or bfloat16 (fp16 has no loss scaling here)"


def weights_init(m):
    """the reference's `apply` hook (discriminator.py:7-13): conv weights N(0, 0.02), BatchNorm weight N(1, 0.02), BatchNorm bias 0"""
    classname = m.__class__.__name__
    if classname.find("Conv") != -1:
        nn.init.normal_(m.weight.data, 0.0, 0.02)
    elif classname.find("BatchNorm") != -1:
        nn.init.normal_(m.weight.data, 1.0, 0.02)
        nn.init.constant_(m.bias.data, 0)


class _Layer:
    """one convolution of `main` with what follows it: its BatchNorm2d holder (or None) and whether a LeakyReLU closes the layer"""

    def __init__(self, conv, norm, act):
        self.conv, self.norm, self.act = conv, norm, act
        s = conv.stride[0]
        self.site = ConvSite(conv, ops.ConvGeom(kh=4, kw=4, sh=s, sw=s, ph=1, pw=1, ph_hi=1, pw_hi=1))
        self.geom, self.cin, self.cout = self.site.geom, self.site.cin, self.site.cout


class NLayerDiscriminator(nn.Module):
    """PatchGAN discriminator (reference discriminator.py:88-137) on gfx950: Conv2d k4 s2 + LeakyReLU(0.2), n_layers - 1 times Conv2d k4 s2
    (no bias) + BatchNorm2d + LeakyReLU, one Conv2d k4 s1 + BatchNorm2d + LeakyReLU, Conv2d k4 s1 -> 1 logit per patch."""

    def __init__(self, input_nc=3, ndf=64, n_layers=3, use_actnorm=False):
        super().__init__()
        if use_actnorm:
            raise NotImplementedError("vidtok_amd NLayerDiscriminator: use_actnorm=True (ActNorm) is not available; the shipped configs use BatchNorm2d")
        if ndf % 8 != 0 or ndf <= 0 or ndf * min(2 ** n_layers, 8) > 512:
            raise ValueError(f"vidtok_amd NLayerDiscriminator: ndf={ndf}: a positive multiple of 8 with at most 512 channels in the widest layer")
        if not 1 <= input_nc <= 8:
            raise ValueError(f"vidtok_amd NLayerDiscriminator: input_nc={input_nc}: 1 .. 8 (the first layer reads an 8-lane stored input)")
        kw, padw = 4, 1
        sequence = [nn.Conv2d(input_nc, ndf, kernel_size=kw, stride=2, padding=padw), nn.LeakyReLU(SLOPE, True)]
        nf_mult = 1
        for n in range(1, n_layers):
            nf_mult_prev, nf_mult = nf_mult, min(2 ** n, 8)
            sequence += [nn.Conv2d(ndf * nf_mult_prev, ndf * nf_mult, kernel_size=kw, stride=2, padding=padw, bias=False),
                         nn.BatchNorm2d(ndf * nf_mult), nn.LeakyReLU(SLOPE, True)]
        nf_mult_prev, nf_mult = nf_mult, min(2 ** n_layers, 8)
        sequence += [nn.Conv2d(ndf * nf_mult_prev, ndf * nf_mult, kernel_size=kw, stride=1, padding=padw, bias=False),
                     nn.BatchNorm2d(ndf * nf_mult), nn.LeakyReLU(SLOPE, True)]
        sequence += [nn.Conv2d(ndf * nf_mult, 1, kernel_size=kw, stride=1, padding=padw)]
        self.main = nn.Sequential(*sequence)
        self.input_nc = input_nc
        self.compute_dtype = torch.float32
        self.last_dtype = None                       # arithmetic of the most recent pass
        mods = list(self.main)
        layers = []
        for i, m in enumerate(mods):
            if isinstance(m, nn.Conv2d):
                norm = mods[i + 1] if i + 1 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm2d) else None
                layers.append(_Layer(m, norm, i + 1 < len(mods)))
        object.__setattr__(self, "_layers", layers)   # plain objects beside the holders: no state_dict key
        self._consts = {}

    # ---- weights ---------------------------------------------------------------------------------------------------------
    @classmethod
    def from_checkpoint(cls, path, prefix="loss.discriminator.", **kw):
        """the discriminator of a published Lightning checkpoint (a local file): the `state_dict` entries under `prefix`, strict"""
        sd = torch.load(path, map_location="cpu", weights_only=True)
        sd = sd.get("state_dict", sd)
        own = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
        if not own:
            raise KeyError(f"{path}: no key starts with {prefix!r}")
        mod = cls(**kw)
        mod.load_state_dict(own, strict=True)
        return mod

    def _apply(self, fn, *a, **kw):
        self._consts = {}
        return super()._apply(fn, *a, **kw)

    def set_compute_dtype(self, dtype):
        """arithmetic of the convolutions outside an autocast region: torch.float32 (default) or torch.bfloat16"""
        if dtype == torch.float16:
            raise NotImplementedError(f"NLayerDiscriminator: {_FP16_MSG}")
        if dtype not in _MODES:
            raise ValueError(f"NLayerDiscriminator compute dtype {dtype}: one of {_MODES}")
        self.compute_dtype = dtype
        return self

    def _dtype_now(self, x):
        on, adt = ops.autocast_state(x.device.type)
        dt = adt if on else self.compute_dtype
        if dt not in _MODES:
            raise NotImplementedError(f"NLayerDiscriminator: {_FP16_MSG}" if dt == torch.float16 else f"NLayerDiscriminator: compute dtype {dt}: float32 or bfloat16")
        return dt

    def _forward_pack(self, i, dt):
        """(packed rows, fp32 bias or None) of convolution i for vt_conv, repacked when the parameter's version changes"""
        return self._layers[i].site.rows(dt, 8 if i == 0 else None)

    def _const(self, c, device):
        """(zeros, ones) fp32 [c]: the identity statistics of a layer without a norm"""
        key = (c, str(device))
        v = self._consts.get(key)
        if v is None:
            v = self._consts[key] = (torch.zeros(c, dtype=torch.float32, device=device), torch.ones(c, dtype=torch.float32, device=device))
        return v

    # ---- the pass --------------------------------------------------------------------------------------------------------
    def _check(self, x, what):
        if x.dim() != 4 or x.shape[1] != self.input_nc:
            raise NotImplementedError(f"NLayerDiscriminator.{what}: input {tuple(x.shape)}: NCHW [N,{self.input_nc},H,W] frames only (flatten a clip to (b t) c h w first)")
        dt = self._dtype_now(x)
        if x.dtype != torch.float32:
            raise TypeError(f"NLayerDiscriminator.{what}: fp32 frames, got {x.dtype}")
        if not x.is_cuda:
            raise L.VtError(f"NLayerDiscriminator.{what}: tensor is on {x.device}; vidtok_amd runs on the GPU only (no CPU fallback)")
        return dt

    def _run(self, x, dt, keep=None):
        """the launches of one pass; `keep` (a list) receives per layer (input, conv output or None, mean, rstd, batch mode)"""
        N, _, H, W = x.shape
        h = ops.ncthw_to_ndhwc(x.detach().contiguous().unsqueeze(2), dt, ld=8)           # [N, 1, H, W, 8]
        last = len(self._layers) - 1
        for i, ly in enumerate(self._layers):
            w, b = self._forward_pack(i, dt)
            if i == last:
                y = ops.conv(h, w, b, ly.geom, cout=ly.cout, out_layout=L.VT_NCTHW)     # fp32 [N, 1, 1, h, w]
                if keep is not None:
                    keep.append((h, None, None, None, False))
                return y.reshape(N, 1, y.shape[3], y.shape[4])
            c = ops.conv(h, w, b, ly.geom, cout=ly.cout)
            zeros, ones = self._const(ly.cout, x.device)
            if ly.norm is None:
                a = ops.batchnorm_act(c, zeros, ones, ones, zeros, SLOPE)
                if keep is not None:
                    keep.append((h, None, None, None, False))
            else:
                bn = ly.norm
                gamma, beta = bn.weight.detach().float().contiguous(), bn.bias.detach().float().contiguous()
                M = c.numel() // c.shape[-1]
                if self.training:
                    if M <= 1:
                        raise ValueError(f"Expected more than 1 value per channel when training, got input size {[N, ly.cout, c.shape[2], c.shape[3]]}")
                    mean, var, rstd = ops.batchnorm_stats(c, eps=bn.eps)
                    with torch.no_grad():
                        mom = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked.item() + 1)
                        bn.running_mean.lerp_(mean.to(bn.running_mean.dtype), mom)
                        bn.running_var.lerp_((var * (M / (M - 1))).to(bn.running_var.dtype), mom)
                        bn.num_batches_tracked += 1
                else:
                    mean = bn.running_mean.detach().float().contiguous()
                    rstd = torch.rsqrt(bn.running_var.detach().float() + bn.eps)
                a = ops.batchnorm_act(c, mean, rstd, gamma, beta, SLOPE)
                if keep is not None:
                    keep.append((h, c, mean, rstd, self.training))
            h = a
        raise AssertionError("unreachable")

    @torch.no_grad()
    def forward(self, x):
        """reference NLayerDiscriminator.forward: fp32 NCHW frames [N,3,H,W] on the GPU -> fp32 logits [N,1,h,w]"""
        dt = self._check(x, "forward")
        self.last_dtype = dt
        return self._run(x, dt)

    def forward_with_grad(self, x):
        """`forward(x)` attached to autograd: the same launches and the same bits, with every layer's input and convolution output kept for
        a backward on the HIP kernels (vt_conv_dgrad, vt_conv_wgrad, vt_batchnorm_act_backward, vt_leaky_relu_backward).  x.grad is
        filled when x requires grad (the generator step), the gradient of every parameter that requires grad is filled (the
        discriminator step; a frozen parameter costs no launch).  With x detached and every parameter frozen it returns the plain value."""
        dt = self._check(x, "forward_with_grad")
        params = [p for p in self.parameters() if p.requires_grad]
        if not torch.is_grad_enabled() or not (x.requires_grad or params):
            return self.forward(x)
        return _PatchGanFunction.apply(self, dt, x, *params)

    def _backward(self, tape, cot, need_dx):
        """-> (dx fp32 NCHW or None, {parameter: gradient}) from the cotangent of the logits"""
        dt, x_shape, kept = tape
        N, _, H, W = x_shape
        grads = {}
        d = ops.grad_ncthw_to_ndhwc(cot.reshape(N, 1, 1, cot.shape[-2], cot.shape[-1]).contiguous().float(), dt, ld=8)
        for i in range(len(self._layers) - 1, -1, -1):
            ly = self._layers[i]
            inp, c, mean, rstd, batch = kept[i]
            if ly.norm is not None:
                bn = ly.norm
                gamma, beta = bn.weight.detach().float().contiguous(), bn.bias.detach().float().contiguous()
                d, dg, db = ops.batchnorm_act_backward(c, d, mean, rstd, gamma, beta, SLOPE, batch=batch, need_dgamma=bn.weight.requires_grad,
                                                       need_dbeta=bn.bias.requires_grad)
                if dg is not None:
                    grads[bn.weight] = dg
                if db is not None:
                    grads[bn.bias] = db
            elif ly.act:
                d = ops.leaky_relu_backward(d, kept[i + 1][0], SLOPE)      # the next layer's input is this layer's post-activation
            elif d.dtype != dt:
                raise AssertionError(d.dtype)
            wreq = ly.conv.weight.requires_grad
            breq = ly.conv.bias is not None and ly.conv.bias.requires_grad
            if wreq or breq:
                dw, dbias = ops.conv_wgrad(inp, d, ly.geom, cin=ly.cin, cout=ly.cout, bias=breq)
                if wreq:
                    grads[ly.conv.weight] = dw.reshape(ly.conv.weight.shape)
                if breq:
                    grads[ly.conv.bias] = dbias
            if not need_dx and not any(p.requires_grad for l2 in self._layers[:i] for p in _layer_params(l2)):
                return None, grads
            d = ly.site.dgrad(d, in_hw=tuple(inp.shape[2:4]), dx_dtype=torch.float32)
        return ops.ndhwc_to_ncthw(d, self.input_nc).reshape(x_shape), grads


def _layer_params(ly):
    out = [ly.conv.weight]
    if ly.conv.bias is not None:
        out.append(ly.conv.bias)
    if ly.norm is not None:
        out += [ly.norm.weight, ly.norm.bias]
    return out


class _PatchGanFunction(torch.autograd.Function):
    """NLayerDiscriminator.forward_with_grad as one autograd node: inputs (x, *trainable parameters), output the logits"""

    @staticmethod
    def forward(ctx, mod, dt, x, *params):
        mod.last_dtype = dt
        kept = []
        val = mod._run(x, dt, keep=kept)
        ctx.mod, ctx.tape, ctx.params = mod, (dt, tuple(x.shape), kept), params
        return val

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, cot):
        if ctx.tape is None:
            raise RuntimeError("NLayerDiscriminator.forward_with_grad: backward through the graph a second time: the saved activations have been freed")
        need_dx = ctx.needs_input_grad[2]
        dx, grads = ctx.mod._backward(ctx.tape, cot, need_dx)
        ctx.tape = None
        return (None, None, dx) + tuple(grads.get(p) for p in ctx.params)
