"""Arena harness: run one launch with every operand carved out of a single allocation, then look at the bytes around them.

An *arena* is one uint8 allocation filled with 0xFF (a NaN as bf16 / fp16 / fp32, -1 as int32).  Operands are *slots* of it; in front of
and behind every slot lies a *moat* of 0xFF bytes, and every slot starts at an ODD multiple of 16 bytes -- (data_ptr() & 31) == 16, the
weakest alignment include/vidtok_amd.h allows, never the 512 bytes of a torch allocation.  After the launch `Arena.check()` asserts on raw
bytes (so NaN compares equal):

  (a) every moat is still 0xFF;
  (b) every input slot holds the bytes that were copied in;
  (c) the pad lanes Cout .. ld-1 of every output row the launch owns are, lane by lane, unchanged (0xFF) or zero;
  (d) output rows the launch does not own (the other parity of an interleaved output, all of y under a fused LayerNorm that does not
      keep it) are unchanged;
  (e) the owned part of every output is, bit for bit, what the same launch wrote into plain torch allocations (or, for the few
      operators that are not reproducible run to run, finite and inside that operator's gate: `compare`).

`relocate(entry)` does the carving for one item of ops.CONV_RECORD and returns the arena with a copy of the descriptor that points
into it; (f), the plan of the relocated descriptor equals the plan of the original, is asserted by the caller (it needs the library).

Nothing here needs a GPU: tests/test_arena_host.py runs the same checks on a CPU arena with plain Python "launches"."""
import ctypes as C
from dataclasses import dataclass
from typing import Callable, Optional

import torch

MOAT = 1 << 20            # the least moat, bytes
FILL = 0xFF
CONV_POINTERS = ("x", "w", "bias", "y", "res", "cache", "mix_factor", "ln_gamma", "ln_beta", "ln_out", "work")
CONV_OUTPUTS = ("y", "ln_out", "work")
TBLOCK_OUTPUTS = ("y", "n_out")
TBLOCK_INOUT = ("cache1", "cache2")


class ArenaError(AssertionError):
    pass


def reach_bytes(t: torch.Tensor) -> int:
    """how far past (or in front of) this operand a tap or a tail tile of a listed shape may read: one frame + one pixel row of a
    [B, T, H, W, C] (or [B, C, T, H, W]) activation; 256 rows (the tallest tile) of a matrix; a vector's own size"""
    es = t.element_size()
    if t.dim() >= 4:
        frame = 1
        for v in t.shape[2:]:
            frame *= int(v)
        row = 1
        for v in t.shape[3:]:
            row *= int(v)
        return (frame + row) * es
    if t.dim() >= 2:
        return min(t.numel(), 256 * int(t.shape[-1])) * es
    return min(t.numel() * es, MOAT // 2)


def _bytes(t: torch.Tensor) -> torch.Tensor:
    assert t.is_contiguous()
    return t.reshape(-1).view(torch.uint8)


@dataclass
class Slot:
    name: str
    kind: str                       # "in" | "out" | "inout" | "scratch"
    nbytes: int
    reach: int
    src: Optional[torch.Tensor] = None        # bytes copied in ("in", "inout")
    expect: Optional[torch.Tensor] = None     # bytes of the plain run ("out", "inout")
    es: int = 1
    row_bytes: int = 0              # "out": ld * es (0: one row = the whole slot)
    real_bytes: int = 0             # "out": Cout * es
    owned: Optional[torch.Tensor] = None      # "out": bool [rows], None = every row
    compare: Optional[Callable] = None        # "out": compare(got_bytes, expect_bytes) raises on a miss; replaces bit equality in (e)
    off: int = -1


class Arena:
    def __init__(self, device="cpu", moat: int = MOAT):
        assert moat >= MOAT, "a moat is at least 1 MiB"
        self.device, self.moat, self.slots, self.buf = torch.device(device), int(moat), {}, None

    # -- declaring slots ------------------------------------------------------------------------------------------------------
    def _add(self, s: Slot):
        assert self.buf is None, "declare every slot before build()"
        if s.name in self.slots:
            raise ArenaError(f"slot {s.name}: declared twice")
        if self.moat < 2 * s.reach:
            raise ArenaError(f"slot {s.name}: moat of {self.moat} bytes is smaller than 2 x (frame + row) = {2 * s.reach} bytes of this operand")
        self.slots[s.name] = s
        return s

    def input(self, name, t: torch.Tensor, reach=None):
        return self._add(Slot(name, "in", t.numel() * t.element_size(), reach_bytes(t) if reach is None else reach, src=_bytes(t)))

    def inout(self, name, before: torch.Tensor, after: torch.Tensor, reach=None):
        assert before.shape == after.shape and before.dtype == after.dtype
        return self._add(Slot(name, "inout", before.numel() * before.element_size(), reach_bytes(before) if reach is None else reach,
                              src=_bytes(before), expect=_bytes(after)))

    def output(self, name, expect: torch.Tensor, *, ld=None, c=None, owned=None, compare=None, reach=None):
        """expect: the plain run's tensor.  ld / c: rows of ld elements of which the first c are real (default: dense).  owned: bool
        [rows] -- rows this launch fills; the others must stay 0xFF."""
        es = expect.element_size()
        n = expect.numel() * es
        row = n if ld is None else ld * es
        real = row if c is None else c * es
        if n % max(row, 1) or real > row:
            raise ArenaError(f"slot {name}: {n} bytes are not whole rows of {row} bytes ({real} real)")
        if owned is not None:
            owned = owned.reshape(-1).to(self.device)
            assert owned.dtype == torch.bool and owned.numel() == n // row, (owned.shape, n // row)
        return self._add(Slot(name, "out", n, reach_bytes(expect) if reach is None else reach, expect=_bytes(expect), es=es, row_bytes=row,
                              real_bytes=real, owned=owned, compare=compare))

    def scratch(self, name, nbytes: int, reach=0):
        """memory the launch may fill with anything (split-K partials, a y that is never read): only its moats are checked"""
        return self._add(Slot(name, "scratch", int(nbytes), reach))

    # -- carving ---------------------------------------------------------------------------------------------------------------
    def build(self):
        cur = 0
        for s in self.slots.values():
            cur += self.moat
            s.off = (cur + 31) // 32 * 32 + 16
            cur = s.off + s.nbytes
        self.buf = torch.full((cur + self.moat + 32,), FILL, dtype=torch.uint8, device=self.device)
        if self.buf.data_ptr() & 31:
            raise ArenaError("the arena itself must start on a 32-byte boundary")
        for s in self.slots.values():
            assert (self.ptr(s.name) & 31) == 16
            if s.src is not None:
                self.raw(s.name).copy_(s.src)
        return self

    def raw(self, name) -> torch.Tensor:
        s = self.slots[name]
        return self.buf[s.off:s.off + s.nbytes]

    def ptr(self, name) -> int:
        return self.buf.data_ptr() + self.slots[name].off

    def view(self, name, dtype, shape) -> torch.Tensor:
        return self.raw(name).view(dtype).view(shape)

    def moats(self):
        """[(start, end, slot before or None, slot after or None)] of the 0xFF bytes between the slots"""
        out, prev, cur = [], None, 0
        for s in self.slots.values():
            out.append((cur, s.off, prev, s))
            prev, cur = s, s.off + s.nbytes
        out.append((cur, self.buf.numel(), prev, None))
        return out

    # -- checking --------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _first(bad: torch.Tensor):
        """index of the first True of a flat mask, or None"""
        if not bool(bad.any()):
            return None
        return int(torch.nonzero(bad.reshape(-1))[0])

    def check(self):
        for a, b, before, after in self.moats():                                                # (a)
            assert b - a >= self.moat
            i = self._first(self.buf[a:b] != FILL)
            if i is not None:
                past = f"slot {before.name}: byte written at offset {before.nbytes + i} (+{i} past its end)" if before is not None else None
                front = f"slot {after.name}: byte written at offset {i - (b - a)} ({b - a - i} before its start)" if after is not None else None
                near_prev = before is not None and (after is None or i < (b - a) // 2)
                raise ArenaError(f"moat touched -- {past if near_prev else front} [value {int(self.buf[a + i])}]")
        for s in self.slots.values():
            got = self.raw(s.name)
            if s.kind == "in":                                                                  # (b)
                i = self._first(got != s.src.to(self.device))
                if i is not None:
                    raise ArenaError(f"slot {s.name}: input byte changed at offset {i}")
            elif s.kind == "inout":
                i = self._first(got != s.expect.to(self.device))
                if i is not None:
                    raise ArenaError(f"slot {s.name}: in/out byte at offset {i} differs from the plain run")
            elif s.kind == "out":
                self._check_output(s, got)

    def _check_output(self, s: Slot, got: torch.Tensor):
        rows = s.nbytes // s.row_bytes if s.row_bytes else 0
        if rows == 0:
            return
        got2 = got.view(rows, s.row_bytes)
        exp2 = s.expect.to(self.device).view(rows, s.row_bytes)
        own = torch.ones((rows,), dtype=torch.bool, device=self.device) if s.owned is None else s.owned
        where = lambda i: f"offset {i} (row {i // s.row_bytes}, lane {(i % s.row_bytes) // s.es})"      # noqa: E731
        i = self._first((got2 != FILL) & ~own[:, None])                                          # (d)
        if i is not None:
            raise ArenaError(f"slot {s.name}: a row this launch does not own was written at {where(i)}")
        if s.real_bytes < s.row_bytes:                                                           # (c)
            pad = got2[:, s.real_bytes:].reshape(rows, -1, s.es)
            kept, zero = (pad == FILL).all(dim=2), (pad == 0).all(dim=2)
            bad = ~(kept | zero) & own[:, None]
            i = self._first(bad)
            if i is not None:
                r, lane = divmod(i, bad.shape[1])
                raise ArenaError(f"slot {s.name}: pad lane neither unchanged nor zero at {where(r * s.row_bytes + s.real_bytes + lane * s.es)}")
        if s.compare is not None:                                                                # (e), gated
            s.compare(got, s.expect.to(self.device))
            return
        bad = (got2[:, :s.real_bytes] != exp2[:, :s.real_bytes]) & own[:, None]                  # (e)
        i = self._first(bad)
        if i is not None:
            r, col = divmod(i, s.real_bytes)
            o = r * s.row_bytes + col
            e0 = o // s.es * s.es
            nan = " -- 0xFF bytes: a moat or an unwritten element reached the result" if bool((got[e0:e0 + s.es] == FILL).all()) else ""
            raise ArenaError(f"slot {s.name}: result differs from the plain run at {where(o)}{nan}")


# ---- relocating one recorded launch ------------------------------------------------------------------------------------------
def _tensors(keep):
    for t in keep:
        if isinstance(t, torch.Tensor):
            yield t
        elif isinstance(t, (tuple, list)):
            yield from _tensors(t)


def _by_pointer(keep):
    out = {}
    for t in _tensors(keep):
        out.setdefault(t.data_ptr(), t)
    return out


def _copy_desc(d):
    d2 = type(d)()
    C.memmove(C.byref(d2), C.byref(d), C.sizeof(d))
    return d2


def _owned_rows(d, t, paired):
    """bool [rows] of an NDHWC output [B, To * yt_mul, Ho * ys_mul, Wo * ys_mul, ld]: the rows the launch d fills (None = all)"""
    tm, sm = max(1, d.yt_mul), max(1, d.ys_mul)
    if paired or (tm == 1 and sm == 1) or t.dim() != 5:
        return None
    _B, TT, HH, WW, _ = t.shape
    assert (TT, HH, WW) == (d.To * tm, d.Ho * sm, d.Wo * sm), (tuple(t.shape), tm, sm)
    ft = torch.arange(TT) % tm == d.yt_off
    fh = torch.arange(HH) % sm == (d.ys_oh if sm > 1 else 0)
    fw = torch.arange(WW) % sm == (d.ys_ow if sm > 1 else 0)
    m = ft[:, None, None] & fh[None, :, None] & fw[None, None, :]
    return m[None].expand(t.shape[0], TT, HH, WW).reshape(-1)


def relocate(entry, plan=None, pre=None, device=None, vt_ncthw=1):
    """entry = (descriptor, kept tensors, label) of ops.CONV_RECORD -> (arena, the descriptor pointing into it).
    plan: ops.conv_plan of a conv descriptor with a LayerNorm (says whether y is written).  pre = {data_ptr: tensor}: what an in/out
    operand held BEFORE the plain run (the kept tensor holds what the run left)."""
    d, keep, _label = entry
    pre = pre or {}
    if isinstance(d, tuple):                                         # ("flash", q, k, vT, bias, o, scale)
        _, q, k, vT, bias, o, scale = d
        ar = Arena(device or q.device, _moat_for([q, k, vT, bias, o]))
        for n, t in (("q", q), ("k", k), ("vT", vT), ("bias", bias)):
            if t is not None:
                ar.input(n, t)
        ar.output("o", o, ld=o.shape[-1], c=o.shape[-1])
        ar.build()
        v = lambda n, t: None if t is None else ar.view(n, t.dtype, t.shape)      # noqa: E731
        return ar, ("flash", v("q", q), v("k", k), v("vT", vT), v("bias", bias), v("o", o), scale)
    tensors = _by_pointer(keep)
    if hasattr(d, "v_ptr") and d.v_ptr:
        fields = list(CONV_POINTERS) + ["v_ptr"]
    elif hasattr(d, "ln_out"):
        fields = list(CONV_POINTERS)
    else:
        fields = [n for n, ty in d._fields_ if ty is C.c_void_p]
    used = {}
    for f in fields:
        p = getattr(d, f)
        if not p:
            continue
        if p not in tensors:
            raise ArenaError(f"descriptor field {f} = {p:#x} points into no kept tensor")
        used.setdefault(p, []).append(f)
    ar = Arena(device or next(iter(tensors.values())).device, _moat_for([tensors[p] for p in used]))
    is_conv = hasattr(d, "ln_out")
    paired = is_conv and bool(getattr(d, "v_ptr", None))
    for p, names in used.items():
        t, name = tensors[p], "/".join(names)
        outs = [n for n in names if n in (CONV_OUTPUTS if is_conv else TBLOCK_OUTPUTS)]
        if not outs:
            if not is_conv and names[0] in TBLOCK_INOUT:
                if p not in pre:
                    raise ArenaError(f"slot {name}: an in/out operand needs its bytes from before the plain run (pre)")
                ar.inout(name, pre[p], t)
            else:
                ar.input(name, t)
            continue
        if len(names) > 1:
            raise ArenaError(f"fields {name} share one tensor but are not all inputs")
        f = names[0]
        if f == "work":
            if t.numel() * t.element_size() != d.work_bytes:
                raise ArenaError(f"slot work: {t.numel() * t.element_size()} bytes kept, {d.work_bytes} in the descriptor")
            ar.scratch(f, d.work_bytes, reach_bytes(t))
        elif not is_conv:
            ar.output(f, t, ld=d.ld, c=d.C)
        elif d.out_layout == vt_ncthw:
            ar.output(f, t)
        else:
            ld = d.ldy if f == "y" else d.ldn
            owned = _owned_rows(d, t, paired)
            if f == "y" and d.ln_mode != 0 and not d.ln_keep_y:
                assert plan is not None, "relocate needs the plan of a launch with a LayerNorm"
                if not plan["ln_fused"]:                             # y is the scratch the separate LayerNorm launch reads
                    ar.scratch(f, t.numel() * t.element_size(), reach_bytes(t))
                    continue
                owned = torch.zeros((t.numel() // ld,), dtype=torch.bool)        # the fused kernel never writes it
            ar.output(f, t, ld=ld, c=d.Cout, owned=owned)
    ar.build()
    d2 = _copy_desc(d)
    for p, names in used.items():
        for f in names:
            setattr(d2, f, ar.ptr("/".join(names)))
    if paired:
        d2.ldv = d.ldv
    return ar, d2


def _moat_for(ts):
    need = max([2 * reach_bytes(t) for t in ts if t is not None] + [MOAT])
    return (need + 31) // 32 * 32


# ---- operators that keep no launch record: log the C calls of a plain ops.* run, replay them with arena pointers -----------------
class CallLog:
    """with CallLog("vt_layernorm_act") as calls: ops.layernorm_act(...)  ->  calls = [(name, args)], the library calls of those names
    exactly as ops.py made them (the plain run itself is not changed)"""

    def __init__(self, *names):
        self.names, self.calls = set(names), []

    def __enter__(self):
        from vidtok_amd import lib as L

        self._L, self._load, real, log = L, L.load, L.load(), self

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(real, name)
                if name not in log.names:
                    return fn

                def call(*args):
                    log.calls.append((name, args))
                    return fn(*args)

                return call

        proxy = Proxy()
        L.load = lambda path=None: proxy
        return self.calls

    def __exit__(self, *exc):
        self._L.load = self._load
        return False


def _pointer_value(a):
    return a.value if isinstance(a, C.c_void_p) else a


def relocate_calls(calls, signatures, operands, scratch=None, device=None):
    """calls: [(name, args)] from CallLog; signatures: lib.SIGNATURES; operands: [dict(name=, t=, kind="in" | "out" | "inout", and for
    outputs ld=, c=, owned=, compare=; for inout before=)] -- every non-null pointer argument (and every pointer field of a descriptor
    argument) must point INTO one of them (an offset into the tensor is kept).  scratch = {argument index: bytes}: a pointer to memory
    the wrapper allocated for the call (a descriptor's `work` is sized by its `work_bytes`).  The last argument is the stream.
    -> (arena, [(name, args pointing into the arena)])"""
    scratch = scratch or {}
    ar = Arena(device or operands[0]["t"].device, _moat_for([o["t"] for o in operands]))
    spans = []
    for o in operands:
        t, kind = o["t"], o.get("kind", "in")
        if kind == "in":
            ar.input(o["name"], t)
        elif kind == "inout":
            ar.inout(o["name"], o["before"], t)
        else:
            ar.output(o["name"], t, ld=o.get("ld"), c=o.get("c"), owned=o.get("owned"), compare=o.get("compare"))
        spans.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), o["name"]))

    def find(p, what):
        for a, b, name in spans:
            if a <= p < b:
                return name, p - a
        raise ArenaError(f"{what} = {p:#x} points into no operand")

    plans = []
    for ci, (name, args) in enumerate(calls):
        types = signatures[name][1]
        assert len(types) == len(args), (name, len(types), len(args))
        plan = []
        for i, (ty, a) in enumerate(zip(types, args)):
            if i == len(args) - 1:
                plan.append(("keep", a))
            elif ty is C.c_void_p:
                p = _pointer_value(a)
                if not p:
                    plan.append(("keep", None))
                elif i in scratch:
                    sname = f"work{ci}.{i}"
                    ar.scratch(sname, scratch[i])
                    plan.append(("ptr", sname, 0))
                else:
                    plan.append(("ptr",) + find(p, f"{name} argument {i}"))
            elif hasattr(a, "_obj") and isinstance(a._obj, C.Structure):
                d, fields = a._obj, []
                for f, fty in d._fields_:
                    p = getattr(d, f)
                    if fty is not C.c_void_p or not p:
                        continue
                    if f == "work":
                        sname = f"work{ci}.{i}"
                        ar.scratch(sname, d.work_bytes)
                        fields.append((f, sname, 0))
                    else:
                        fields.append((f,) + find(p, f"{name} descriptor field {f}"))
                plan.append(("desc", d, fields))
            else:
                plan.append(("keep", a))
        plans.append((name, plan))
    ar.build()
    out = []
    for name, plan in plans:
        args = []
        for item in plan:
            if item[0] == "keep":
                args.append(item[1])
            elif item[0] == "ptr":
                args.append(C.c_void_p(ar.ptr(item[1]) + item[2]))
            else:
                d2 = _copy_desc(item[1])
                for f, sname, off in item[2]:
                    setattr(d2, f, ar.ptr(sname) + off)
                ar._keep = getattr(ar, "_keep", []) + [d2]
                args.append(C.byref(d2))
        out.append((name, tuple(args)))
    return ar, out
