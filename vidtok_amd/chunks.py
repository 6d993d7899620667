"""Where the chunk-to-chunk state of a v1.1 pass lives on the Python host, and who writes it (csrc/model.cpp keeps the same state in
CState / TileScope / SessionSwap).  Every caching module owns a `Slot` and only reads it and rebinds its cache; an encoder or a decoder
owns one `ChunkState` over the slots below it, and the engine and the sessions write nothing else.  Plain objects next to the modules:
no `state_dict` key, no buffer, and a deep copy or pickle of a module tree carries its own."""
import torch


class Slot:
    """what one caching module carries from chunk to chunk: `cache` (a tensor or None), `offset` (frames at the end of the chunk
    that the kept state skips: the look-ahead of an overlapped decode) and the persistent buffers the cache lives in"""

    def __init__(self):
        self.state = _ALONE
        self.cache = None
        self.offset = 0
        self.bufs = {}

    first = property(lambda self: self.state.first)
    tiled = property(lambda self: self.state.tiled)

    def persistent(self, shape, like):
        """The cache lives in one buffer per (slot, shape, dtype, device), allocated on first use and rewritten in place afterwards:
        a chunk of a given kind reads and writes the same addresses every time, which is what lets a captured chunk
        (vidtok_amd/graphs.py) be replayed.  `cache` is bound to the buffer after each update and reset to None between clips;
        `bufs` survives the reset."""
        key = (tuple(shape), like.dtype, like.device)
        buf = self.bufs.get(key)
        if buf is None:
            buf = self.bufs[key] = torch.empty(tuple(shape), dtype=like.dtype, device=like.device)
        return buf


def slots_of(module):
    """the slots under `module`, in module.modules() order"""
    return [m.slot for m in module.modules() if isinstance(getattr(m, "slot", None), Slot)]


class ChunkState:
    """The state of one encoder or decoder over the chunks of a pass: `first` (the first chunk, or a whole clip), `tiled` (chunks
    follow one another, so every block leaves its caches behind; False lets a block that can run as ONE launch keep its convolutions'
    inputs on chip), `overlap` (chunks carry a look-ahead latent frame: `overlap_table` holds each slot's offset then, None where the
    factor is refused) and the slots of `part`."""

    def __init__(self, part=None):
        # a block built on its own reads these defaults (_ALONE): the first chunk, caches kept as the reference's modules keep them
        self.first, self.tiled, self.overlap = True, True, False
        self.slots = slots_of(part) if part is not None else []
        self.overlap_table = None
        for s in self.slots:
            s.state = self

    def reset(self, drop_buffers=False):
        """between clips: no cache bound; the buffers stay while captured chunks replay against them"""
        for s in self.slots:
            s.cache = None
            if drop_buffers:
                s.bufs.clear()

    def set_overlap(self, on):
        """every pass says which: the overlapped table, or zeros"""
        assert not on or self.overlap_table is not None, "Only support 2x, 4x or 8x temporal downsampling now."
        self.overlap = bool(on)
        for s, off in zip(self.slots, self.overlap_table if on else [0] * len(self.slots)):
            s.offset = off

    def caches(self):
        """[(slot, its cache)]: what a captured chunk leaves bound, re-applied by `bind` after a replay (which runs no Python)"""
        return [(s, s.cache) for s in self.slots]

    @staticmethod
    def bind(caches):
        for s, c in caches:
            s.cache = c

    def sig(self):
        """how many frames each cache holds right now (part of a chunk kind's graph key)"""
        return tuple(0 if s.cache is None else s.cache.shape[1] for s in self.slots)

    def snapshot(self):
        return self.first, self.tiled, self.overlap, [(s.cache, s.offset) for s in self.slots]

    def restore(self, snap):
        self.first, self.tiled, self.overlap, per_slot = snap
        for s, (cache, offset) in zip(self.slots, per_slot):
            s.cache, s.offset = cache, offset


_ALONE = ChunkState()
