"""Weight re-packing: reference parameter layouts -> the [Cout][taps*Cin_p] rows vt_conv reads.

The reference stores nn.Conv3d / Conv2d / Conv1d weights as [Cout, Cin, kT, kH, kW] /
[Cout, Cin, kH, kW] / [Cout, Cin, k] (state_dict shapes listed in SURVEY.md section 8b).  vt_conv wants
k = ((kt*KH + kh)*KW + kw)*Cin_p + c contiguous per output channel, in the arithmetic dtype,
with Cin zero-padded to the activation's stored channel count.  Packing is a one-time permute /
pad / cast done with torch tensor ops (data movement only) and cached per (dtype, version).
"""
import torch

from . import lib as L
from . import ops
from .ops import pad_channels


def pack_conv_weight(weight: torch.Tensor, dtype: torch.dtype, cin_stored: int = None) -> torch.Tensor:
    """weight [Cout, Cin, *k] (1, 2 or 3 kernel dims) -> [Cout, taps * cin_stored] contiguous."""
    cout, cin = weight.shape[:2]
    cin_p = cin_stored or pad_channels(cin)
    nd = weight.dim() - 2
    w = weight.detach().to(torch.float32)
    # channels-last: [Cout, *k, Cin]
    perm = (0,) + tuple(range(2, 2 + nd)) + (1,)
    w = w.permute(*perm)
    if cin_p != cin:
        w = torch.nn.functional.pad(w, (0, cin_p - cin))
    return w.reshape(cout, -1).to(dtype).contiguous()


ARITH_SPLIT3 = "bf16x3"
SPLIT3_DTYPE = torch.int32        # element type of a split-bf16 weight container (4 bytes per k, like the fp32 row it replaces)


def pack_split3(w2d: torch.Tensor) -> torch.Tensor:
    """Packed fp32 rows [Cout, K] -> the operand of vt_conv's VT_BF16X3 arithmetic (include/vidtok_amd.h): every value as
    two bf16 planes, hi = bf16(w) (round to nearest even) and lo = bf16(w - hi), stored per group of 16 k as
    [hi 16 x bf16 | lo 16 x bf16] (64 bytes, the size of the 16 fp32 values they replace), K zero-padded to 32 (a whole
    128-byte K step of the kernel).  Returned as an INT32-typed container [Cout, K32] (ldw = K32): the element type is the
    tag ops.conv reads (`SPLIT3_DTYPE`) -- unlike a Python attribute it survives .view / .contiguous / slicing, and a
    split container can never be taken for fp32 rows.  Data movement + two roundings."""
    cout, K = w2d.shape
    Kp = (K + 31) // 32 * 32
    w = w2d.detach().to(torch.float32)
    if Kp != K:
        w = torch.nn.functional.pad(w, (0, Kp - K))
    hi = w.to(torch.bfloat16)
    lo = (w - hi.to(torch.float32)).to(torch.bfloat16)
    planes = torch.stack([hi.view(cout, Kp // 16, 16), lo.view(cout, Kp // 16, 16)], dim=2).contiguous()   # [Cout, K/16, 2, 16]
    return planes.view(SPLIT3_DTYPE).reshape(cout, Kp)


def packed_caches(root: torch.nn.Module):
    """every PackedCache under `root`.  The one rule: a cache belongs to a ConvSite, and a module keeps its sites as attributes, directly
    or inside tuples / lists"""
    def visit(v):
        if isinstance(v, ConvSite):
            yield v.pack
        elif isinstance(v, (tuple, list)):
            for e in v:
                yield from visit(e)

    for m in root.modules():
        for v in vars(m).values():
            yield from visit(v)


def set_arith(root: torch.nn.Module, arith):
    """Select the weight arithmetic of every convolution under `root` for fp32 storage: None = fp32 rows (fp32 MFMA),
    ARITH_SPLIT3 = split-bf16 planes (three bf16 MFMAs per product).  Caches created with pin_native=True (operands of an
    activation x activation GEMM) keep fp32 rows."""
    assert arith in (None, ARITH_SPLIT3)
    for cache in packed_caches(root):
        if not cache.pin_native:
            cache.arith = arith


def time_upsample_parity_weights(weight: torch.Tensor, early: bool):
    """A k=3 temporal conv over a nearest-x2 frame-repeated input u[t] = x[t >> 1] touches only two input frames per
    output frame, so it equals a k=2 conv over x with pre-summed taps (fp32 sums, rounded once when packed):
      window (j-1, j)  when the three taps cover u[2j-2 .. 2j]   : [W0 + W1, W2]   `early=True`
                       or                 u[2j-1 .. 2j+1] causal : [W0, W1 + W2]   `early=False`
    (the caller pairs each output parity with its window, see TimeUpsampleRes*2x).  weight [Co, Ci, 3, kh, kw]."""
    w = weight.detach().to(torch.float32)
    assert w.dim() == 5 and w.shape[2] == 3
    if early:
        return torch.stack([w[:, :, 0] + w[:, :, 1], w[:, :, 2]], dim=2)
    return torch.stack([w[:, :, 0], w[:, :, 1] + w[:, :, 2]], dim=2)


def space_upsample_parity_weights(weight: torch.Tensor, py: int, px: int):
    """A 3x3 conv (pad 1) over a nearest-x2 up-sampled frame v[Y][X] = x[Y>>1][X>>1] reads, for an output pixel of
    parity (py, px), only a 2x2 window of x: rows (a-1, a) with taps [W0, W1+W2] for py = 0, rows (a, a+1) with
    [W0+W1, W2] for py = 1, likewise for columns.  weight [Co, Ci, 3, 3] -> [Co, Ci, 2, 2] (fp32 sums)."""
    w = weight.detach().to(torch.float32)
    assert w.dim() == 4 and tuple(w.shape[2:]) == (3, 3)
    rows = torch.stack([w[:, :, 0], w[:, :, 1] + w[:, :, 2]], dim=2) if py == 0 else \
        torch.stack([w[:, :, 0] + w[:, :, 1], w[:, :, 2]], dim=2)                     # [Co, Ci, 2, 3]
    return torch.stack([rows[..., 0], rows[..., 1] + rows[..., 2]], dim=3) if px == 0 else \
        torch.stack([rows[..., 0] + rows[..., 1], rows[..., 2]], dim=3)               # [Co, Ci, 2, 2]


def time_upsample_parity_mix(kdims, early: bool):
    """the tap sums of time_upsample_parity_weights as a mix table for vt_pack_conv_weight: kdims = (3, kh, kw) of the reference
    weight -> 2 * kh * kw output taps, each [m0, m1] (indices into the 3 * kh * kw reference taps)"""
    kt, kh, kw = kdims
    assert kt == 3
    s = kh * kw
    first = [[0 * s + i, 1 * s + i] if early else [0 * s + i] for i in range(s)]
    second = [[2 * s + i] if early else [1 * s + i, 2 * s + i] for i in range(s)]
    return first + second


def time_upsample3_weights(weight: torch.Tensor, part: str):
    """The causal v1.0 time up-sampler as three frame products (vt_time_upsample3): with x[-1] = 0
      o[2j] = U[j] + V[j-1],  o[2j+1] = U[j] + V[j],   U[j] = W0 x[j-1] + W2 x[j],  V[j] = W1 x[j]
    part "u": the k=2 window [W0, W2] over (x[j-1], x[j]); part "v": W1 alone, a per-frame kh x kw convolution.  No tap is summed: every
    tap is the reference's, rounded once when packed.  weight [Co, Ci, 3, kh, kw] -> [Co, Ci, 2, kh, kw] / [Co, Ci, 1, kh, kw]."""
    w = weight.detach().to(torch.float32)
    assert w.dim() == 5 and w.shape[2] == 3 and part in ("u", "v")
    if part == "u":
        return torch.stack([w[:, :, 0], w[:, :, 2]], dim=2)
    return w[:, :, 1:2]


def time_upsample3_mix(kdims, part: str):
    """time_upsample3_weights as a mix table for vt_pack_conv_weight: (3, kh, kw) -> 2 * kh * kw (u) or kh * kw (v) single taps"""
    kt, kh, kw = kdims
    assert kt == 3 and part in ("u", "v")
    s = kh * kw
    if part == "u":
        return [[0 * s + i] for i in range(s)] + [[2 * s + i] for i in range(s)]
    return [[1 * s + i] for i in range(s)]


def space_upsample_parity_mix(kdims, py: int, px: int):
    """the tap sums of space_upsample_parity_weights as a mix table: (3, 3) -> 4 output taps (r, c), each (w[r0][c0] + w[r1][c0]) +
    (w[r0][c1] + w[r1][c1]) over its row set and column set -- rows first, then columns, as the host statement sums them"""
    assert tuple(kdims) == (3, 3)
    rows = [[0], [1, 2]] if py == 0 else [[0, 1], [2]]
    cols = [[0], [1, 2]] if px == 0 else [[0, 1], [2]]
    out = []
    for R in rows:
        for Cc in cols:
            m = [-1, -1, -1, -1]
            for ci, c in enumerate(Cc):
                for ri, r in enumerate(R):
                    m[2 * ci + ri] = r * 3 + c
            out.append(m)
    return out


class PackedCache:
    """Caches the packed weight / fp32 bias of one conv-like parameter holder.  `transform` (optional) maps the
    parameter tensor to the tensor that is packed (e.g. the parity weights of a time up-sampler); `mix` is the same
    transform as a tap-sum table (kernel dims -> [[m0..m3], ...]) for the device packer.  Parameters that live on the GPU
    are packed there by vt_pack_conv_weight (same bits as the host statements; no foreign kernel in the process);
    host parameters (CPU tests, tools) by the torch statements above."""

    def __init__(self, transform=None, pin_native=False, mix=None):
        self._entries = {}           # (dtype, arith, cin_stored) -> (validity key, (w, b)): the packed rows of every mode the module has run
        self._transform = transform  # in stay alive, so a graph captured in one mode still replays after a detour through another
        self._mix = mix
        assert (transform is None) == (mix is None)
        self.arith = None            # set_arith(): ARITH_SPLIT3 = fp32 requests are answered with split-bf16 planes
        self.pin_native = pin_native

    def get(self, weight: torch.nn.Parameter, bias, dtype, cin_stored=None):
        arith = self.arith if dtype == torch.float32 else None
        key = (dtype, weight.device, weight._version, None if bias is None else bias._version, cin_stored,
               weight.data_ptr(), arith)
        slot = (dtype, arith, cin_stored)
        ent = self._entries.get(slot)
        if ent is None or ent[0] != key:
            if weight.is_cuda:
                wd = weight.detach()
                wd = wd if wd.dtype == torch.float32 and wd.is_contiguous() else wd.float().contiguous()
                mix = None if self._mix is None else self._mix(tuple(wd.shape[2:]))
                w = ops.pack_conv_weight(wd, dtype, cin_stored, mix=mix, split3=arith == ARITH_SPLIT3)
            else:
                w = pack_conv_weight(weight if self._transform is None else self._transform(weight), dtype, cin_stored)
                if arith == ARITH_SPLIT3:
                    w = pack_split3(w)
            b = None if bias is None else bias.detach().to(torch.float32).contiguous()
            ent = self._entries[slot] = (key, (w, b))
        return ent[1]


class DgradPackCache:
    """The transposed, tap-flipped rows vt_conv_dgrad convolves dy with (ops.pack_conv_weight_dgrad: one block per parity class of the
    geometry's strides), cached per parameter version like PackedCache: an optimizer step bumps `weight._version` and the next backward
    packs again.  GPU parameters only (the backward has no host form)."""

    def __init__(self, geom):
        self._geom = {} if (geom.sh, geom.sw) == (1, 1) else {"geom": geom}      # stride 1: the plain rows [Cin, ldw]
        self._entries = {}           # (dtype, cout_stored) -> (validity key, rows)

    def get(self, weight: torch.nn.Parameter, dtype, cout_stored):
        key = (weight.device, weight._version, weight.data_ptr())
        slot = (dtype, cout_stored)
        ent = self._entries.get(slot)
        if ent is None or ent[0] != key:
            wd = weight.detach()
            wd = wd if wd.dtype == torch.float32 and wd.is_contiguous() else wd.float().contiguous()
            ent = self._entries[slot] = (key, ops.pack_conv_weight_dgrad(wd, dtype, cout_stored, **self._geom))
        return ent[1]


class ConvSite:
    """One convolution as the kernels see it: the parameter holder (nn.Conv1d / Conv2d / Conv3d, never called), the geometry of its launch and
    the packed forms of its weight.  A plain object, built in the __init__ of the module that runs it, so it adds no state_dict key and a
    copy of the module copies it along with the holder.  Several sites may share a holder: the parity classes of an up-sampler, the W_v
    row operand of attention.  `clip_tmode` is the time-pad mode on a whole clip (what the training path runs); chunked passes hand `run`
    their own mode and cache (CausalConv3d / CausalConv1d)."""

    def __init__(self, conv, geom, *, clip_tmode=L.VT_TPAD_ZERO, transform=None, mix=None, pin_native=False, bias=True):
        self.conv, self.geom, self.clip_tmode = conv, geom, clip_tmode
        self.bias = bias             # False: the site runs without the holder's bias (one of several terms of the holder's convolution)
        self.cin, self.cout = conv.in_channels, conv.out_channels
        self.pack = PackedCache(transform, pin_native, mix)
        self._dgrad = None           # DgradPackCache, made by the first backward

    def rows(self, dt, cin_stored):
        """(packed weight rows, fp32 bias) alone, for the launches that are not ops.conv"""
        return self.pack.get(self.conv.weight, self.conv.bias if self.bias else None, dt, cin_stored=cin_stored)

    def run(self, x, dt, *, tmode=L.VT_TPAD_ZERO, cache=None, **kw):
        w, b = self.rows(dt, x.shape[-1])
        return ops.conv(x, w, b, self.geom, cout=self.cout, tmode=tmode, cache=cache, **kw)

    def run_clip(self, x, dt, **kw):
        return self.run(x, dt, tmode=self.clip_tmode, **kw)

    def dgrad_rows(self, dtype, cout_stored):
        if self._dgrad is None:
            self._dgrad = DgradPackCache(self.geom)
        return self._dgrad.get(self.conv.weight, dtype, cout_stored)

    def dgrad(self, dy, *, in_hw=None, **kw):
        """dx of the site's convolution on a whole clip (ops.conv_dgrad); in_hw: the input's (Hi, Wi), read under a stride only"""
        if (self.geom.sh, self.geom.sw) != (1, 1):
            kw["in_hw"] = in_hw
        return ops.conv_dgrad(dy, self.dgrad_rows(dy.dtype, dy.shape[-1]), self.geom, cin=self.cin, cout=self.cout, tmode=self.clip_tmode, **kw)


# ---- parity classes of a convolution's data gradient (vt_conv_dgrad, include/vidtok_amd.h) --------------------------------------------
def strided_axis_class(k: int, s: int, p: int, r: int, extent: int = None) -> dict:
    """one axis of a parity class: input positions i = s j + r receive the taps k0, k0 + s, ... (those with (r + p - tap) mod s = 0)
    from dy[j + (r + p) // s - m] for the m-th of them.  As a stride-1 convolution over dy that is the flipped tap list under the front
    pad nk - 1 - (r + p) // s.  -> dict(r, taps (forward tap indices in flipped order, as the class kernel walks them), pad, n (class
    extent, with `extent`))"""
    k0 = (r + p) % s
    taps = list(range(k0, k, s))
    out = dict(r=r, taps=taps[::-1], pad=len(taps) - 1 - (r + p) // s)
    if extent is not None:
        out["n"] = (extent - r + s - 1) // s if extent > r else 0
    return out


def strided_dgrad_classes(kh: int, kw: int, sh: int, sw: int, ph: int, pw: int, hi: int = None, wi: int = None) -> list:
    """the class table of vt_conv_dgrad, class rh * sw + rw at index rh * sw + rw: [(rows, cols)] of strided_axis_class.  Every forward
    tap (p, q) appears in exactly one class (stride 1: the one class holds them all, flipped, under the mirrored pads K - 1 - p); a
    negative pad -- every class with an empty tap list (K < s) has one -- is a geometry the entry point refuses."""
    return [(strided_axis_class(kh, sh, ph, rh, hi), strided_axis_class(kw, sw, pw, rw, wi)) for rh in range(sh) for rw in range(sw)]
