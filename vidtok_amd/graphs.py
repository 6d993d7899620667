"""Per-shape hipGraph cache for the encoder / decoder launch sequences.

An encode or decode of one clip batch is 150-250 kernel launches issued from Python; eager, the host paces the GPU
(measured round 1: FSQ 559 frames/s eager vs 680 captured).  `GraphedCall` wraps a pure device function
`f(x) -> tensor` (EncoderCausal3DPadding.forward, DecoderCausal3DPadding.forward): the first call of a shape runs
eagerly (it also packs the weights), the second is captured into a hipGraph on a side stream, later calls copy the
input into the graph's static buffer and replay.  Outputs are returned as fresh tensors (a device-to-device copy of the
graph's static output), so the reference's "caller owns the outputs" contract holds.

Opt-in (`AutoencodingEngine.enable_graphs()`): a replay runs no host code, so it would not see in-place edits of parameters
made after the capture (the packed weight copies are refreshed only when Python asks for them).  `version_fn`, when given,
returns a fingerprint of the parameters the function reads (their `_version` counters, which every in-place update such as
`optimizer.step()` bumps); a call that finds it changed drops the captured graphs first.  `load_state_dict`, `.to()`,
`set_compute_dtype` and `enable_graphs` reset the cache as well; edits that bypass the version counter (`p.data = ...`)
need `invalidate_graphs()`.  A call site keeps at most `GraphedCall.MAX_ENTRIES` shapes (least recently used out first) and its
graphs share one memory pool, so a process that sees many clip lengths / resolutions does not accumulate working sets.

Stateful chunked passes (v1.1 temporal tiling) replay too: the modules keep their chunk-to-chunk caches in persistent
buffers that are updated in place (vidtok_amd/chunks.py::Slot.persistent), so a captured chunk reads and writes the same
addresses on every replay.  Such a call (`stateful=True`) must run exactly once per chunk: the usual side-stream warm-up
run before the capture is skipped (the first, eager call of the shape already packed the weights), and capturing does
not execute.  `frames=(start, end)` passes the chunk as a frame range of a larger NCTHW fp32 tensor (copied straight
into the graph's input by vt_ncthw_copy_frames); `borrow=True` returns the graph's own output tensor -- valid until the
next call of the same shape -- instead of a copy.
"""
import torch


class GraphedCall:
    MAX_ENTRIES = 12     # shapes / chunk kinds kept per call site; the least recently used one is dropped beyond that

    def __init__(self, fn, state_get=None, state_set=None, version_fn=None):
        self.fn = fn
        self.entries = {}
        self.version_fn = version_fn
        self._version = None
        # stateful calls: host-side state the function leaves behind (module attributes bound to cache buffers), read
        # after the capture and re-applied after every replay -- a replay runs no Python
        self.state_get, self.state_set = state_get, state_set
        # one memory pool for all graphs of this call site: they never run concurrently, and what a caller may still
        # hold of a graph (its static input / output) stays allocated as long as the entry lives
        self._pool = None

    def clear(self):
        self.entries.clear()
        self._pool = None

    # a copy / pickle of the owner starts with an empty cache (graphs hold device state and are not copyable)
    def __deepcopy__(self, memo):
        import copy

        return GraphedCall(copy.deepcopy(self.fn, memo), copy.deepcopy(self.state_get, memo), copy.deepcopy(self.state_set, memo),
                           copy.deepcopy(self.version_fn, memo))

    def __getstate__(self):
        return {"fn": self.fn, "state_get": self.state_get, "state_set": self.state_set, "version_fn": self.version_fn}

    def __setstate__(self, st):
        self.__init__(st["fn"], st["state_get"], st["state_set"], st.get("version_fn"))

    @staticmethod
    def _is_stateful(e):
        return isinstance(e, tuple) and e[3] is not None

    @property
    def overfull(self):
        """more entries than MAX_ENTRIES: only stateful ones can pile up (see _touch); the owner resets between passes"""
        return len(self.entries) > self.MAX_ENTRIES

    def _touch(self, key):
        """LRU bookkeeping: `key` becomes the most recent entry; beyond MAX_ENTRIES the oldest stateless entries go.
        Stateful entries replay against addresses they captured (the modules' persistent chunk-cache buffers) in the
        middle of a chunked pass, so they are never dropped from here: the owner checks `overfull` between passes and
        resets everything together with those buffers (AutoencodingEngineV11._empty_causal_cached)."""
        self.entries[key] = self.entries.pop(key)
        for old in list(self.entries):
            if len(self.entries) <= self.MAX_ENTRIES:
                break
            if old != key and not self._is_stateful(self.entries[old]):
                del self.entries[old]

    # the device side of a call, as four small methods: bench.py's host-loop self-test (--selftest-steps) runs the REAL
    # __call__ below -- key construction, cache lookup, LRU bookkeeping, state hand-over -- with these stubbed out
    def _on_device(self, x):
        return x.is_cuda

    def _fill(self, dst, x, frames):
        if frames is None:
            return dst.copy_(x)
        from . import ops

        return ops.ncthw_copy_frames(x, dst, frames[0], 0, frames[1] - frames[0])

    def _replay(self, g):
        """hipGraphLaunch through the C-ABI (vt_graph_launch).  torch's CUDAGraph.replay() first refreshes the seed / offset of
        every registered device generator -- two fill kernels per replay -- which the captured sequences never read (no random
        numbers are drawn on the device: the KL noise is the reference's host stream)."""
        ex = getattr(g, "_vt_exec", None)
        if ex is None:
            g.replay()
            return
        import ctypes as C

        from . import lib as L

        L.check(L.load().vt_graph_launch(C.c_void_p(ex), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "vt_graph_launch")

    def _result(self, sy, borrow):
        return sy if borrow else sy.clone()

    def __call__(self, x, key_extra=(), stateful=False, frames=None, borrow=False):
        if not self._on_device(x):
            return self.fn(x if frames is None else x[:, :, frames[0]:frames[1]].contiguous())
        if self.version_fn is not None:
            v = self.version_fn()
            if v != self._version:          # parameters updated in place since the capture: the graphs replay stale weights
                self.clear()
                self._version = v
        x = x.contiguous()
        if frames is not None:
            x = x.float()
            shape = tuple(x.shape[:2]) + (frames[1] - frames[0],) + tuple(x.shape[3:])
        else:
            shape = tuple(x.shape)

        def fill(dst):
            return self._fill(dst, x, frames)

        key = (shape, x.dtype, x.device, key_extra)
        e = self.entries.get(key)
        if e is None:                       # first sight of this shape: eager (packs weights, sizes the allocator)
            y = self.fn(x if frames is None else fill(torch.empty(shape, dtype=x.dtype, device=x.device)))
            self.entries[key] = "warm"
            self._touch(key)
            return y
        if e == "warm":
            sx = fill(torch.empty(shape, dtype=x.dtype, device=x.device))
            if not stateful:
                cur = torch.cuda.current_stream()
                side = torch.cuda.Stream()
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    self.fn(sx)
                cur.wait_stream(side)
            if self._pool is None:
                self._pool = torch.cuda.graph_pool_handle()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self._pool):
                sy = self.fn(sx)
            try:                            # the instantiated graph's handle, for vt_graph_launch (older torch: replay() of the wrapper)
                g._vt_exec = int(g.raw_cuda_graph_exec()) or None
            except (AttributeError, RuntimeError):
                g._vt_exec = None
            self.entries[key] = e = (g, sx, sy, self.state_get() if stateful and self.state_get else None)
        self._touch(key)
        g, sx, sy, state = e
        fill(sx)
        self._replay(g)
        if state is not None:
            self.state_set(state)
        return self._result(sy, borrow)
