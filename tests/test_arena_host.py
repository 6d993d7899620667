"""The arena harness (tests/arena.py) on the CPU: the detector must detect.  The "launch" is a plain Python function on arena views --
y[b, 2t + off] = x[b, t] * 2 into the frames of one parity of an interleaved [B, 2T, H, W, ld] output with ld = C + 8 -- and every
mutant of it (a store past the slot, in front of it, into a pad lane, into a frame of the other parity, into an input, a result
computed from a moat byte) has to be reported with the slot's name and the byte offset."""
import ctypes as C
import re

import pytest
import torch

import arena as A

B, T, H, W, CH, LD = 2, 3, 4, 5, 8, 16
OFF = 1                                    # this launch owns the odd frames
DT = torch.bfloat16
ES = 2
ROW = LD * ES


def _plain():
    """operands and the plain run's result (the other parity's frames are whatever the allocation held: here zeros)"""
    g = torch.Generator().manual_seed(1)
    x = torch.randn((B, T, H, W, CH), generator=g).to(DT)
    y = torch.zeros((B, 2 * T, H, W, LD), dtype=DT)
    y[:, OFF::2, :, :, :CH] = x * 2
    return x, y


def _owned():
    m = torch.zeros((B, 2 * T, H, W), dtype=torch.bool)
    m[:, OFF::2] = True
    return m


def _arena():
    x, y = _plain()
    ar = A.Arena("cpu")
    ar.input("x", x)
    ar.output("y", y, ld=LD, c=CH, owned=_owned())
    return ar.build(), x, y


def _launch(ar, zero_pads=False):
    xv = ar.view("x", DT, (B, T, H, W, CH))
    yv = ar.view("y", DT, (B, 2 * T, H, W, LD))
    yv[:, OFF::2, :, :, :CH] = xv * 2
    if zero_pads:
        yv[:, OFF::2, :, :, CH:] = 0


def _reported(ar, slot, offset):
    with pytest.raises(A.ArenaError) as e:
        ar.check()
    msg = str(e.value)
    assert f"slot {slot}:" in msg, msg
    nums = [int(v) for v in re.findall(r"offset (-?\d+)", msg)]
    assert offset in nums, (offset, msg)
    return msg


def test_placement_is_an_odd_multiple_of_16_bytes_with_whole_moats():
    ar, _x, _y = _arena()
    assert ar.buf.dtype == torch.uint8 and ar.buf.data_ptr() % 32 == 0
    for name in ("x", "y"):
        assert ar.ptr(name) & 31 == 16
        assert ar.view(name, DT, (-1,)).data_ptr() == ar.ptr(name)
    gaps = ar.moats()
    assert len(gaps) == 3 and all(b - a >= A.MOAT for a, b, _p, _n in gaps)
    assert all(bool((ar.buf[a:b] == 0xFF).all()) for a, b, _p, _n in gaps)
    assert bool((ar.raw("y") == 0xFF).all()) and torch.isnan(ar.view("y", DT, (-1,)).float()).all()
    assert torch.equal(ar.view("x", DT, (B, T, H, W, CH)), _plain()[0])
    assert int(ar.raw("y").view(torch.int32)[0]) == -1


def test_moat_must_cover_twice_a_frame_and_a_row():
    big = torch.zeros((1, 2, 64, 64, 128), dtype=DT)              # one frame = 1 MiB: the default moat is too small
    assert A.reach_bytes(big) == (64 * 64 * 128 + 64 * 128) * 2
    with pytest.raises(A.ArenaError, match=r"slot big: moat of 1048576 bytes is smaller than 2 x \(frame \+ row\) = 2129920"):
        A.Arena("cpu").input("big", big)
    A.Arena("cpu", moat=2 * A.reach_bytes(big)).input("big", big)
    with pytest.raises(AssertionError):
        A.Arena("cpu", moat=4096)                                    # never less than 1 MiB


def test_correct_launch_passes():
    ar, _x, _y = _arena()
    _launch(ar)
    ar.check()                       # pad lanes left unchanged
    ar, _x, _y = _arena()
    _launch(ar, zero_pads=True)
    ar.check()                       # pad lanes zero-filled


def test_an_unwritten_output_is_reported():
    ar, _x, _y = _arena()
    msg = _reported(ar, "y", 1 * H * W * ROW)                        # the first owned row is frame 1 of clip 0
    assert "0xFF" in msg


def test_store_past_the_slot():
    ar, _x, y = _arena()
    _launch(ar)
    n = y.numel() * ES
    end = ar.slots["y"].off + n
    ar.buf[end + 6] = 0                                              # one element, three elements past the last row
    ar.buf[end + 7] = 0
    _reported(ar, "y", n + 6)


def test_store_in_front_of_the_slot():
    ar, _x, _y = _arena()
    _launch(ar)
    ar.buf[ar.slots["x"].off - 2] = 0x3F
    msg = _reported(ar, "x", -2)
    assert "before its start" in msg
    ar, _x, _y = _arena()                                            # in front of the second slot, nearer to it than to x's end
    _launch(ar)
    ar.buf[ar.slots["y"].off - 32] = 1
    _reported(ar, "y", -32)


def test_store_into_a_pad_lane():
    ar, _x, _y = _arena()
    _launch(ar, zero_pads=True)
    yv = ar.view("y", DT, (B, 2 * T, H, W, LD))
    yv[1, 3, 2, 1, CH + 3] = 1.5
    row = ((1 * 2 * T + 3) * H + 2) * W + 1
    _reported(ar, "y", row * ROW + (CH + 3) * ES)
    ar, _x, _y = _arena()                                            # half an element zeroed is neither unchanged nor zero
    _launch(ar)
    ar.raw("y")[OFF * H * W * ROW + CH * ES] = 0
    _reported(ar, "y", OFF * H * W * ROW + CH * ES)


def test_store_into_a_frame_of_the_other_parity():
    ar, _x, _y = _arena()
    _launch(ar)
    yv = ar.view("y", DT, (B, 2 * T, H, W, LD))
    yv[0, 2, 0, 0, 1] = 0.0                                          # frame 2 belongs to the launch with offset 0
    msg = _reported(ar, "y", 2 * H * W * ROW + 1 * ES)
    assert "does not own" in msg
    ar, _x, _y = _arena()                                            # ... its pad lanes too: an un-owned row stays as it was, every byte
    _launch(ar)
    ar.view("y", DT, (B, 2 * T, H, W, LD))[1, 0, 3, 4, LD - 1] = 0.0
    _reported(ar, "y", (((1 * 2 * T) * H + 3) * W + 4) * ROW + (LD - 1) * ES)


def test_changed_input_byte():
    ar, _x, _y = _arena()
    _launch(ar)
    ar.raw("x")[77] ^= 0x10
    msg = _reported(ar, "x", 77)
    assert "input byte changed" in msg


def test_result_computed_from_a_moat_byte():
    """a gather one element past x: the last real lane of the last pixel reads the moat -> NaN in y"""
    ar, _x, _y = _arena()
    xs = ar.slots["x"]
    xv = ar.buf[xs.off + ES:xs.off + ES + xs.nbytes].view(DT).view(B, T, H, W, CH)          # the over-reading view
    yv = ar.view("y", DT, (B, 2 * T, H, W, LD))
    _launch(ar)
    yv[-1, -1, -1, -1, :CH] = torch.cat([xv[-1, -1, -1, -1, CH - 1:], ar.view("x", DT, (B, T, H, W, CH))[-1, -1, -1, -1, 1:]]) * 2     # lane 0 from the moat
    assert torch.isnan(yv[-1, -1, -1, -1, 0].float())
    _reported(ar, "y", ar.slots["y"].nbytes - ROW)
    # ... a wrong but finite element is reported as well, without that remark
    ar2, _x, _y = _arena()
    _launch(ar2)
    ar2.view("y", DT, (B, 2 * T, H, W, LD))[0, OFF, 0, 0, 0] += 1
    _reported(ar2, "y", OFF * H * W * ROW)


def test_gated_compare_replaces_bit_equality_but_not_the_other_checks():
    x, y = _plain()
    seen = []

    def gate(got, exp):
        seen.append(1)
        g, e = got.view(DT).float().view(B, 2 * T, H, W, LD)[:, OFF::2, :, :, :CH], exp.view(DT).float().view(B, 2 * T, H, W, LD)[:, OFF::2, :, :, :CH]
        if not (torch.isfinite(g).all() and (g - e).abs().max() <= 0.05):
            raise A.ArenaError("slot y: outside the gate")

    def mk():
        ar = A.Arena("cpu")
        ar.input("x", x)
        ar.output("y", y, ld=LD, c=CH, owned=_owned(), compare=gate)
        return ar.build()

    ar = mk()
    _launch(ar)
    ar.view("y", DT, (B, 2 * T, H, W, LD))[0, OFF, 0, 0, 0] += 0.01
    ar.check()
    assert seen
    ar = mk()
    _launch(ar)
    ar.view("y", DT, (B, 2 * T, H, W, LD))[0, 0, 0, 0, 0] = 0.0
    with pytest.raises(A.ArenaError, match="does not own"):
        ar.check()


# ---- relocate() on descriptors that point into host tensors ---------------------------------------------------------------------
def _conv_entry(yt=(2, OFF), ln_keep=None):
    from vidtok_amd import lib as L

    x, y = _plain()
    w = torch.ones((CH, CH), dtype=DT)
    bias = torch.zeros((CH,), dtype=torch.float32)
    d = L.ConvDesc()
    d.x, d.w, d.bias, d.y = x.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr()
    d.B, d.To, d.Ho, d.Wo, d.Cin, d.Cout, d.ldy = B, T, H, W, CH, CH, LD
    d.yt_mul, d.yt_off = yt
    d.out_layout = L.VT_NDHWC
    return (d, (x, w, (bias, 1e-6, True), y, None), None), x, y


def test_relocate_carves_every_pointer_field_and_keeps_the_rest_of_the_descriptor():
    (entry, x, y) = _conv_entry()
    ar, d2 = A.relocate(entry)
    d = entry[0]
    assert set(ar.slots) == {"x", "w", "bias", "y"} and [ar.slots[n].kind for n in ("x", "w", "bias", "y")] == ["in", "in", "in", "out"]
    assert (d2.x, d2.w, d2.bias, d2.y) == tuple(ar.ptr(n) for n in ("x", "w", "bias", "y")) and not d2.res and not d2.work
    assert all(getattr(d2, n) == getattr(d, n) for n, ty in d._fields_ if ty is not C.c_void_p)
    assert ar.slots["y"].row_bytes == ROW and ar.slots["y"].real_bytes == CH * ES and torch.equal(ar.slots["y"].owned, _owned().reshape(-1))
    _launch(ar)
    ar.check()
    ar.view("y", DT, (B, 2 * T, H, W, LD))[0, 0, 0, 0, 0] = 0.0
    with pytest.raises(A.ArenaError, match="slot y: a row this launch does not own"):
        ar.check()


def test_relocate_refuses_a_pointer_into_no_kept_tensor():
    (entry, _x, _y) = _conv_entry()
    stray = torch.zeros((4,))
    entry[0].res = stray.data_ptr()
    with pytest.raises(A.ArenaError, match="field res .* points into no kept tensor"):
        A.relocate(entry)


def test_relocate_shares_one_slot_between_fields_that_share_a_tensor_and_sizes_work_exactly():
    (entry, x, _y) = _conv_entry(yt=(1, 0))
    d = entry[0]
    d.res = x.data_ptr()
    work = torch.zeros((1000,), dtype=torch.uint8)
    d.work, d.work_bytes = work.data_ptr(), 1000
    ar, d2 = A.relocate((d, entry[1] + (work,), None))
    assert d2.x == d2.res == ar.ptr("x/res") and ar.slots["work"].kind == "scratch" and ar.slots["work"].nbytes == 1000
    assert ar.slots["y"].owned is None
    d.work_bytes = 999
    with pytest.raises(A.ArenaError, match="slot work"):
        A.relocate((d, entry[1] + (work,), None))


def test_relocate_fused_layernorm_without_y_leaves_y_unowned():
    (entry, _x, y) = _conv_entry(yt=(1, 0))
    d = entry[0]
    n = torch.zeros_like(y)
    g = torch.ones((CH,))
    d.ln_gamma, d.ln_beta, d.ln_out, d.ln_mode, d.ln_keep_y, d.ldn = g.data_ptr(), g.data_ptr(), n.data_ptr(), 2, 0, LD
    e2 = (d, entry[1] + (n, g), None)
    ar, d2 = A.relocate(e2, plan=dict(ln_fused=True))
    assert d2.ln_gamma == d2.ln_beta == ar.ptr("ln_gamma/ln_beta")
    assert not bool(ar.slots["y"].owned.any()) and ar.slots["ln_out"].owned is None
    ar.view("ln_out", DT, y.shape)[..., :CH] = 0
    ar.check()
    ar.raw("y")[5] = 0
    _reported(ar, "y", 5)
    ar, _d2 = A.relocate(e2, plan=dict(ln_fused=False))             # a separate LayerNorm launch reads y: scratch
    assert ar.slots["y"].kind == "scratch"


def test_relocate_temporal_block_needs_the_caches_from_before_the_run():
    from vidtok_amd import lib as L

    x = torch.randn((1, 3, 2, 2, 8)).to(DT)
    y = (x.float() + 1).to(DT)
    c_before, c_after = torch.zeros((1, 2, 2, 2, 8), dtype=DT), x[:, 1:].clone()
    d = L.TBlockDesc()
    d.x, d.y, d.cache1 = x.data_ptr(), y.data_ptr(), c_after.data_ptr()
    d.C = d.ld = 8
    entry = (d, (x, y, (c_after, None)), None)
    with pytest.raises(A.ArenaError, match="slot cache1: an in/out operand"):
        A.relocate(entry)
    ar, d2 = A.relocate(entry, pre={c_after.data_ptr(): c_before})
    assert [s.kind for s in ar.slots.values()] == ["in", "out", "inout"] and d2.cache1 == ar.ptr("cache1") and not d2.cache2
    assert bool((ar.raw("cache1") == 0).all())
    ar.view("y", DT, x.shape).copy_(y)
    ar.view("cache1", DT, c_after.shape).copy_(c_after)
    ar.check()
    ar.raw("cache1")[3] ^= 1
    _reported(ar, "cache1", 3)
