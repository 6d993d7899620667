"""LPIPS (VGG16) on the HIP kernels: the third metric of the reference's eval loop (scripts/inference_evaluate.py:164-186).

`LPIPS` mirrors the reference's `vidtok.modules.lpips.LPIPS` -- same constructor argument `use_dropout`, same submodules, same
`state_dict` keys and shapes (a state_dict saved from the reference loads with strict=True), same `forward(input, target) -> [N,1,1,1]`
on NCHW images in [-1, 1] -- but it never downloads anything: the weights come from two local files (or `load_state_dict`).

The pass over N image pairs (include/vidtok_amd.h, vt_lpips_*): vt_lpips_prep builds one NHWC stack of the 2N scaled frames (input
frames first), every VGG16 conv + ReLU is ONE vt_conv_act launch over both images, vt_lpips_tap runs the fused head of a tap and the
2 x 2 max-pool that feeds the next slice, vt_lpips_finish sums the spatial means.  Arithmetic of the convolutions: fp32 by default
(the reference's eval without --precision autocast), `set_compute_dtype(torch.bfloat16 | torch.float16)`, or the dtype of the
caller's torch.autocast("cuda") region (the reference's precision_scope("cuda")); the head is fp32 in every mode.

`LPIPS.forward_with_grad` is the same pass attached to autograd with respect to the reconstruction, for the perceptual term of the
reference's decoder loss (vidtok/modules/losses.py:173-176): a HIP backward (vt_lpips_tap_backward, vt_conv_dgrad, vt_relu_backward,
vt_lpips_prep_backward) over the reconstruction frames, fp32 or bf16.  Everything else here stays under no_grad.
"""
import os

import torch
import torch.nn as nn

from . import lib as L
from . import ops

CHNS = [64, 128, 256, 512, 512]
# torchvision vgg16().features[0:30] ("D" configuration): index -> (Cin, Cout) of the 3x3 convolutions; ReLU after each, MaxPool2d(2, 2)
# at 4, 9, 16, 23 (and 30, outside the slices)
VGG_CONVS = {0: (3, 64), 2: (64, 64), 5: (64, 128), 7: (128, 128), 10: (128, 256), 12: (256, 256), 14: (256, 256),
             17: (256, 512), 19: (512, 512), 21: (512, 512), 24: (512, 512), 26: (512, 512), 28: (512, 512)}
VGG_POOLS = (4, 9, 16, 23, 30)
SLICES = ((0, 4), (4, 9), (9, 16), (16, 23), (23, 30))           # vgg16.slice1..5 (reference lpips.py:139-148)
TAP_AFTER = {2: 0, 7: 1, 14: 2, 21: 3, 28: 4}                    # the conv whose ReLU is relu1_2 ... relu5_3
DEFAULT_LPIPS_CKPT = os.path.join("checkpoints", "lpips", "vgg.pth")   # the reference's get_ckpt_path("vgg_lpips", "checkpoints/lpips")
VGG16_FILE = "vgg16-397923af.pth"                                # torchvision's vgg16 weights file name under <hub dir>/checkpoints
_GEOM3 = ops.ConvGeom(kh=3, kw=3, ph=1, pw=1, ph_hi=1, pw_hi=1)
_MODES = (torch.float32, torch.bfloat16, torch.float16)


def _slice_of(idx: int) -> int:
    for k, (a, b) in enumerate(SLICES):
        if a <= idx < b:
            return k + 1
    raise KeyError(idx)


def vgg_features_to_lpips(sd: dict) -> dict:
    """torchvision vgg16 state_dict keys features.N.{weight,bias} -> net.sliceK.N.* (other keys, e.g. classifier.*, are dropped)"""
    out = {}
    for k, v in sd.items():
        parts = k.split(".")
        if len(parts) == 3 and parts[0] == "features" and int(parts[1]) in VGG_CONVS:
            out[f"net.slice{_slice_of(int(parts[1]))}.{parts[1]}.{parts[2]}"] = v
    return out


class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.Tensor([-0.030, -0.088, -0.188])[None, :, None, None])
        self.register_buffer("scale", torch.Tensor([0.458, 0.448, 0.450])[None, :, None, None])


class NetLinLayer(nn.Module):
    """1x1 conv C -> 1 without bias; a Dropout in front (key model.1.weight) when use_dropout, as the reference"""

    def __init__(self, chn_in, chn_out=1, use_dropout=False):
        super().__init__()
        layers = [nn.Dropout()] if use_dropout else []
        layers += [nn.Conv2d(chn_in, chn_out, 1, stride=1, padding=0, bias=False)]
        self.model = nn.Sequential(*layers)


class vgg16(nn.Module):
    """the five slices of torchvision's vgg16().features[0:30] (parameters only; the arithmetic is the HIP path of LPIPS)"""

    def __init__(self):
        super().__init__()
        for k, (a, b) in enumerate(SLICES):
            s = nn.Sequential()
            for i in range(a, b):
                if i in VGG_CONVS:
                    s.add_module(str(i), nn.Conv2d(*VGG_CONVS[i], kernel_size=3, padding=1))
                elif i in VGG_POOLS:
                    s.add_module(str(i), nn.MaxPool2d(kernel_size=2, stride=2))
                else:
                    s.add_module(str(i), nn.ReLU(inplace=True))
            setattr(self, f"slice{k + 1}", s)
        for p in self.parameters():
            p.requires_grad = False


class LPIPS(nn.Module):
    """Learned perceptual metric (reference vidtok/modules/lpips.py:64-95) on gfx950.

    pretrained=True loads `lpips_ckpt` (the LPIPS lin-layer file, the reference's checkpoints/lpips/vgg.pth) and `vgg_ckpt` (a
    torchvision vgg16 state_dict; default <torch.hub.get_dir()>/checkpoints/vgg16-397923af.pth, read only).  A missing file raises
    FileNotFoundError naming both paths -- nothing is downloaded.  pretrained=False leaves the parameters uninitialised (tests, or
    a later load_state_dict)."""

    def __init__(self, use_dropout=True, pretrained=True, lpips_ckpt=DEFAULT_LPIPS_CKPT, vgg_ckpt=None):
        super().__init__()
        self.scaling_layer = ScalingLayer()
        self.chns = list(CHNS)
        self.net = vgg16()
        for k, c in enumerate(CHNS):
            setattr(self, f"lin{k}", NetLinLayer(c, use_dropout=use_dropout))
        self.compute_dtype = torch.float32
        self.last_dtype = None                      # arithmetic of the most recent pass (tests: the autocast region's dtype ran)
        self._packs = {}
        if pretrained:
            self.load_pretrained(lpips_ckpt, vgg_ckpt)
        for p in self.parameters():
            p.requires_grad = False

    # ---- weights -----------------------------------------------------------------------------------------------------
    def load_pretrained(self, lpips_ckpt=DEFAULT_LPIPS_CKPT, vgg_ckpt=None):
        vgg_ckpt = vgg_ckpt or os.path.join(torch.hub.get_dir(), "checkpoints", VGG16_FILE)
        missing = [p for p in (lpips_ckpt, vgg_ckpt) if not os.path.isfile(p)]
        if missing:
            raise FileNotFoundError(
                f"LPIPS weights: lin layers {lpips_ckpt!r} ({'missing' if lpips_ckpt in missing else 'found'}), VGG16 features {vgg_ckpt!r} "
                f"({'missing' if vgg_ckpt in missing else 'found'}); vidtok_amd does not download weights -- place both files there, pass "
                "lpips_ckpt= / vgg_ckpt=, or construct with pretrained=False and load_state_dict")
        self.load_state_dict(vgg_features_to_lpips(torch.load(vgg_ckpt, map_location="cpu", weights_only=True)), strict=False)
        self.load_state_dict(torch.load(lpips_ckpt, map_location="cpu", weights_only=True), strict=False)

    def _apply(self, fn, *a, **kw):               # .to() / .cuda() / .half(): the packed copies are stale
        self._packs = {}
        return super()._apply(fn, *a, **kw)

    def load_state_dict(self, *a, **kw):
        self._packs = {}
        return super().load_state_dict(*a, **kw)

    def set_compute_dtype(self, dtype):
        """arithmetic of the convolutions outside an autocast region: torch.float32 (default), torch.bfloat16 or torch.float16"""
        if dtype not in _MODES:
            raise ValueError(f"LPIPS compute dtype {dtype}: one of {_MODES}")
        self.compute_dtype = dtype
        return self

    def _dtype_now(self, x):
        on, adt = ops.autocast_state(x.device.type)
        if on:
            if adt not in (torch.bfloat16, torch.float16):
                raise NotImplementedError(f"vidtok_amd LPIPS under torch.autocast(dtype={adt}): bfloat16 and float16 regions only")
            return adt
        return self.compute_dtype

    def _pack(self, dtype, device):
        key = (dtype, str(device))
        p = self._packs.get(key)
        if p is None:
            convs = []
            for k, (a, b) in enumerate(SLICES):
                s = getattr(self.net, f"slice{k + 1}")
                for i in range(a, b):
                    if i in VGG_CONVS:
                        m = getattr(s, str(i))
                        w = m.weight.detach().to(device=device, dtype=torch.float32).contiguous()
                        bias = m.bias.detach().to(device=device, dtype=torch.float32).contiguous()
                        convs.append((i, ops.pack_conv_weight(w, dtype, cin_stored=8 if i == 0 else None), bias, m.out_channels))
            lins = [getattr(self, f"lin{k}").model[-1].weight.detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous()
                    for k in range(5)]
            shift = self.scaling_layer.shift.detach().to(device=device, dtype=torch.float32).reshape(3).contiguous()
            scale = self.scaling_layer.scale.detach().to(device=device, dtype=torch.float32).reshape(3).contiguous()
            p = self._packs[key] = (convs, lins, shift, scale)
        return p

    def _pack_dgrad(self, dtype, device):
        """the 13 convolutions' weights as vt_conv_dgrad reads them (vt_pack_conv_weight_dgrad), cached beside the forward packs"""
        key = ("dgrad", dtype, str(device))
        p = self._packs.get(key)
        if p is None:
            p = []
            for k, (a, b) in enumerate(SLICES):
                s = getattr(self.net, f"slice{k + 1}")
                for i in range(a, b):
                    if i in VGG_CONVS:
                        w = getattr(s, str(i)).weight.detach().to(device=device, dtype=torch.float32).contiguous()
                        p.append(ops.pack_conv_weight_dgrad(w, dtype, cout_stored=w.shape[0]))
            self._packs[key] = p
        return p

    # ---- the pass ----------------------------------------------------------------------------------------------------
    def _run(self, x, y, dt, flags=0, tap_means=False, keep=None):
        """the launches of one pass in arithmetic `dt`; `keep` (a list) receives every convolution's post-ReLU output [2N,1,h,w,c]"""
        convs, lins, shift, scale = self._pack(dt, x.device)
        x, y = x.float().contiguous(), y.float().contiguous()
        n = x.shape[0] * (x.shape[2] if x.dim() == 5 else 1)
        H, W = x.shape[-2:]
        h = ops.lpips_prep(x, y, shift, scale, dt, flags).unsqueeze(1)      # [2N, 1, H, W, 8]: NDHWC with one frame
        work = torch.empty((ops.lpips_work_bytes(n, H, W) // 4,), dtype=torch.float32, device=x.device)
        for idx, w, b, cout in convs:
            h = ops.conv_act(h, w, b, _GEOM3, cout=cout)
            if keep is not None:
                keep.append(h)
            if idx in TAP_AFTER:
                k = TAP_AFTER[idx]
                pooled = ops.lpips_tap(h[:, 0], lins[k], work, k, pool=k < 4)
                h = pooled.unsqueeze(1) if pooled is not None else None
        return ops.lpips_finish(work, n, H, W, tap_means=tap_means)

    @torch.no_grad()
    def values(self, x, y, flags=0, tap_means=False):
        """LPIPS of every frame pair of x, y (NCHW [N,3,H,W] or NCTHW [B,3,T,H,W], on the GPU) -> fp32 [N] (frame n = b*T + t), and the
        per-tap spatial means [5, N] with tap_means=True.  flags: vidtok_amd.lib.VT_LPIPS_* (clamp of y, eval-loop round trip, [0,1] input)"""
        assert x.shape == y.shape and x.dim() in (4, 5) and x.shape[1] == 3, (x.shape, y.shape)
        dt = self._dtype_now(x)
        self.last_dtype = dt
        return self._run(x, y, dt, flags, tap_means)

    def forward(self, input, target):
        """reference LPIPS.forward: NCHW images in [-1, 1] -> [N, 1, 1, 1]"""
        assert input.dim() == 4
        return self.values(input, target).reshape(-1, 1, 1, 1)

    def frames(self, x, y, eval_loop=True):
        """per-frame LPIPS [B, T] of NCTHW clips x (input) and y (reconstruction) in [-1, 1].  eval_loop: the reference loop's form --
        clamp of y only, then (v + 1) / 2 and LPIPS on v * 2 - 1 (scripts/inference_evaluate.py:175-186)"""
        assert x.dim() == 5
        flags = (L.VT_LPIPS_CLAMP_Y | L.VT_LPIPS_ROUNDTRIP) if eval_loop else 0
        return self.values(x, y, flags).reshape(x.shape[0], x.shape[2])

    # ---- the differentiable pass (decoder fine-tuning) -----------------------------------------------------------------
    def forward_with_grad(self, input, target):
        """`forward(input, target)` attached to autograd with respect to `target` (the reconstruction): the same launches and the same
        bits, with every convolution's post-ReLU output kept for a backward on the HIP kernels (vt_lpips_tap_backward, vt_conv_dgrad,
        vt_relu_backward, vt_lpips_prep_backward) over the N reconstruction frames.  `input` is the ground truth and gets no gradient;
        VGG16 and the lin layers are frozen.  fp32 or bf16 arithmetic; NCHW [N,3,H,W] only.  A target that does not require grad gets
        the plain value."""
        if input.dim() != 4 or target.dim() != 4:
            raise NotImplementedError(f"LPIPS.forward_with_grad: {input.dim()}-D input: NCHW [N,3,H,W] images only (flatten a clip's frames first)")
        dt = self._dtype_now(input)
        if dt not in (torch.float32, torch.bfloat16):
            raise NotImplementedError(f"LPIPS.forward_with_grad: compute dtype {dt}: the backward kernels take float32 or bfloat16 (fp16 has no loss scaling here)")
        if input.requires_grad:
            raise NotImplementedError("LPIPS.forward_with_grad: input.requires_grad: the gradient is taken with respect to target only (input is the ground truth)")
        if target.dtype != torch.float32 or input.shape != target.shape or input.shape[1] != 3:
            raise TypeError(f"LPIPS.forward_with_grad: fp32 [N,3,H,W] pairs of one shape, got {tuple(input.shape)} and {tuple(target.shape)} {target.dtype}")
        for name, t in (("input", input), ("target", target)):
            if not t.is_cuda:
                raise L.VtError(f"LPIPS.forward_with_grad.{name}: tensor is on {t.device}; vidtok_amd runs on the GPU only (no CPU fallback)")
        if not (torch.is_grad_enabled() and target.requires_grad):
            return self.forward(input, target)
        return _LpipsFunction.apply(self, dt, input, target)

    def _backward(self, tape, cot):
        """d(sum(cot * lpips)) / d target, fp32 NCHW: from relu5_3 down over the reconstruction half of the kept features"""
        dt, n, feats = tape
        dev = feats[0].device
        _, lins, _, scale = self._pack(dt, dev)
        wts = self._pack_dgrad(dt, dev)
        gout = cot.reshape(-1).float().contiguous()
        d = None                                    # fp32 gradient at the output of the convolution below (through the pool at a tap)
        for (idx, (cin, cout)), y, wt in reversed(list(zip(VGG_CONVS.items(), feats, wts))):
            if idx in TAP_AFTER:
                dpre = ops.lpips_tap_backward(y[:, 0], lins[TAP_AFTER[idx]], gout, dpool=None if d is None else d[:, 0]).unsqueeze(1)
            else:
                dpre = ops.relu_backward(d, y[n:])
            d = ops.conv_dgrad(dpre, wt, _GEOM3, cin=cin, cout=cout, dx_dtype=torch.float32)
        return ops.lpips_prep_backward(d[:, 0], scale)


class _LpipsFunction(torch.autograd.Function):
    """LPIPS.forward_with_grad as one autograd node: inputs (input, target), output [N,1,1,1]; gradient to target only"""

    @staticmethod
    def forward(ctx, mod, dt, input, target):
        mod.last_dtype = dt
        feats = []
        val = mod._run(input, target, dt, keep=feats)
        ctx.mod, ctx.tape = mod, (dt, input.shape[0], feats)
        return val.reshape(-1, 1, 1, 1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, cot):
        return None, None, None, ctx.mod._backward(ctx.tape, cot)
