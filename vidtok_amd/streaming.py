"""Streaming sessions of the v1.1 causal tokenizers: the temporal tiling of AutoencodingEngineV11 (tile_encode / tile_decode,
autoencoder_v1_1.py:218-331) fed as the frames arrive -- a live feed, a camera, the tokens an autoregressive model emits chunk by
chunk -- instead of from one whole clip on the device.

    enc = model.open_encode_session(t_chunk_enc=16)
    for frames in feed:                       # fp32 [B, C, n, H, W] on the device, any n >= 1
        z, log = enc.push(frames)             # the latents of every chunk this push completed (chunk 0 = the first frame alone)
    z, log = enc.finish()                     # the incomplete last chunk, if any

Contract: the chunk schedule is build_chunk_start_end's ([0,1), [1,1+c), [1+c,1+2c) ...), so for every split of a clip into
pushes the concatenated outputs equal tile_encode / tile_decode bit for bit (KL with host noise: one draw per chunk, in chunk
order -- the generator is consumed as tile_encode consumes it).  A decode session with overlap runs a chunk once the latent after
it has arrived (tile_decode's `look` rule), or at finish.  A ReconstructSession chains both and reports at finish how many
leading frames forward() drops.

Each session owns its causal state.  Captured chunk graphs (engine.enable_graphs) replay against the slots' persistent cache
buffers (chunks.py::Slot.persistent), so a push copies the session's state into those buffers and back out afterwards
-- two vt_copy_segments launches whatever the number of caches -- and restores the snapshot of both halves' chunk states: sessions,
interleaved with each other and with plain model(x) / encode / decode calls, do not see each other.  Device memory is bounded by
the chunk (the frames of the incomplete chunk, the caches), not by the length of the video.
"""
import torch

from . import ops


class ChunkSchedule:
    """build_chunk_start_end, advanced push by push (host logic only).  `step`: chunk length after the single-frame first chunk;
    `lookahead`: a chunk runs once that many frames past its end have arrived (the overlapped decoder: 1), or at finish.
    push(n) / finish() -> [(start, end, look)] of the chunks that became ready, in order, in frames since the first push."""

    def __init__(self, step: int, lookahead: int = 0):
        assert step >= 1 and lookahead in (0, 1)
        self.step, self.lookahead = step, lookahead
        self.received = 0          # frames pushed so far
        self.start = 0             # first frame of the next chunk
        self.index = 0             # chunks emitted so far
        self.finished = False

    def _end(self):
        return self.start + (1 if self.index == 0 else self.step)

    def push(self, n: int):
        if self.finished:
            raise RuntimeError("session: push after finish()")
        if int(n) < 1:
            raise ValueError(f"session: a push takes n >= 1 frames (got {n})")
        self.received += int(n)
        out = []
        while self._end() + self.lookahead <= self.received:
            end = self._end()
            out.append((self.start, end, self.lookahead > 0))
            self.start, self.index = end, self.index + 1
        return out

    def finish(self):
        if self.finished:
            raise RuntimeError("session: finish() called twice")
        self.finished = True
        if self.start >= self.received:
            return []
        out = [(self.start, self.received, False)]       # the last chunk: partial, or complete with nothing after it
        self.start, self.index = self.received, self.index + 1
        return out

    @property
    def pending(self):
        """frames received but not yet part of a chunk that ran"""
        return self.received - self.start


def encode_emission(chunks, f):
    """latent frames that chunks [(start, end, look)] of an encode yield: a chunk of n frames is front-padded to a multiple of f"""
    return sum(-(-(e - s) // f) for s, e, _ in chunks)


def decode_emission(chunks, f):
    """output frames that chunks of a decode yield: f per latent frame (the look-ahead latent's frames are dropped)"""
    return sum(f * (e - s) for s, e, _ in chunks)


def check_sessions_supported(model):
    if getattr(model, "version", None) != "v1_1" or not getattr(model, "is_causal", False):
        raise NotImplementedError(
            f"vidtok_amd: sessions exist only for the v1.1 causal models (this one: version {getattr(model, 'version', '?')}, "
            f"{'causal' if getattr(model, 'is_causal', False) else 'non-causal'}): the reference has no chunk protocol for the others "
            f"(v1.0 long videos: VideoReconstructor's pad_gen_frames chaining)")


class _Session:
    """shared part of the encode / decode sessions: the schedule, the buffer of the incomplete chunk, the session's causal state
    and the switch into / out of the model"""

    _graphed_name = None          # "_genc" | "_gdec"

    def __init__(self, model, part, step, lookahead):
        check_sessions_supported(model)
        self.model, self.part = model, part
        self.f = model.encoder.time_downsample_factor
        self.sched = ChunkSchedule(step, lookahead)
        self.state = part.chunks
        self._saved = [None] * len(self.state.slots)
        self._tables = {}
        self._pend = None
        self._geom = None           # (B, C, H, W) of the first push
        self._mode = None           # the arithmetic the session runs in (fixed at the first push)
        self._out_shape = None
        self.switches = 0

    # ---- bookkeeping -----------------------------------------------------------------------------------------------------
    def _check_input(self, x, what):
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 5):
            raise ValueError(f"{what}: an NCTHW tensor on the GPU (got {type(x).__name__} {getattr(x, 'shape', '')})")
        geom = (x.shape[0], x.shape[1]) + tuple(x.shape[3:])
        if self._geom is None:
            self._geom = geom
        elif geom != self._geom:
            raise ValueError(f"{what}: B / C / H / W {geom} differ from the first push's {self._geom}")

    def _sync_mode(self, x):
        m = self.model
        m._sync_autocast(x)
        mode = (m.arith, self.part.compute_dtype, getattr(self.part, "tail_dtype", None), getattr(self.part, "tail_level", None))
        if self._mode is None:
            self._mode = mode
        elif mode != self._mode:
            raise RuntimeError(f"session: the arithmetic changed in the middle of the session ({self._mode[0]} -> {mode[0]}: autocast "
                               f"region or set_compute_dtype); open a new session for it")

    def _copy(self, pairs):
        """one vt_copy_segments launch for [(src, dst)]; tables are kept per address set (stable between pushes)"""
        if not pairs:
            return
        key = tuple((s.data_ptr(), d.data_ptr(), s.numel() * s.element_size()) for s, d in pairs)
        hit = self._tables.get(key)
        if hit is None:
            if len(self._tables) >= 8:
                self._tables.clear()
            hit = self._tables[key] = ops.segment_table(pairs, pairs[0][0].device)
        ops.copy_segments(*hit)

    # ---- the switch --------------------------------------------------------------------------------------------------------
    def _enter(self):
        self._snap = [st.snapshot() for st in self.model._chunk_states()]     # both halves: _set_first_chunk writes both
        self.state.set_overlap(self.sched.lookahead > 0)      # the decoder's cache offsets of an overlapped pass, else zeros
        self.state.tiled = True                               # blocks keep their chunk state (AutoencodingEngineV11._set_fused_temporal)
        pairs = []
        for slot, saved in zip(self.state.slots, self._saved):
            if saved is None:
                slot.cache = None
                continue
            buf = slot.persistent(saved.shape, saved)
            pairs.append((saved, buf))
            slot.cache = buf
        self._copy(pairs)
        self.switches += 1

    def _leave(self):
        pairs = []
        for i, slot in enumerate(self.state.slots):
            c = slot.cache
            if c is None:
                self._saved[i] = None
                continue
            s = self._saved[i]
            if s is None or s.shape != c.shape or s.dtype != c.dtype:
                s = self._saved[i] = torch.empty_like(c, memory_format=torch.contiguous_format)
            pairs.append((c.contiguous(), s))
        self._copy(pairs)

    def _restore(self):
        for st, snap in zip(self.model._chunk_states(), self._snap):
            st.restore(snap)
        self._snap = None

    # ---- one push --------------------------------------------------------------------------------------------------------
    def _advance(self, n, fill, direct=None):
        """schedule n more frames; `fill(dst, dst_t0, src_t0, count)` stages frames [src_t0, src_t0 + count) of this push into
        `dst` at dst_t0; `direct` (an fp32 NCTHW tensor of this push's frames) lets a chunk that lies wholly inside it run from
        it.  Runs the chunks that became ready; returns their outputs (see _collect)."""
        base = self.sched.received
        chunks = self.sched.push(n) if n is not None else self.sched.finish()
        received = self.sched.received
        if self._pend is None:
            self._alloc_pending()
        outs = []
        if chunks:
            self._enter()
            try:
                for s, e, look in chunks:
                    hi = e + (1 if look else 0)
                    if direct is not None and s >= base:
                        src, t0 = direct, s - base
                    else:
                        lo = max(s, base)         # [s, lo) waits in the buffer since earlier pushes
                        if hi > lo:
                            fill(self._pend, lo - s, lo - base, hi - lo)
                        src, t0 = self._pend, 0
                    outs.append(self._run(src, t0, t0 + hi - s, s == 0, look))
                self._leave()
            finally:
                self._restore()
        # what is left of this push waits for its chunk: frames [start, received) at the front of the buffer
        start = self.sched.start
        lo = max(start, base)
        if received > lo and n is not None:
            fill(self._pend, lo - start, lo - base, received - lo)
        return outs

    def _run(self, src, t0, t1, first, look):
        m = self.model
        m._set_first_chunk(first)
        return m._chunk_call(getattr(m, self._graphed_name), self.part, src, t0, t1, first)

    @property
    def finished(self):
        return self.sched.finished


class EncodeSession(_Session):
    """push(x) / push_u8(frames) / finish() -> (z, log): z fp32 [B, C', n', H', W'] of the chunks the call completed (n' may be
    0), log {"indices": int32 [B, n', H', W'] (FSQ), "chunk_logs": [the regularizer's log of each chunk]}.  `chunk_losses` /
    `reg_log()`: the per-chunk kl_loss / aux_loss and their mean (tile_encode's reg_log)."""

    _graphed_name = "_genc"

    def __init__(self, model, t_chunk_enc=None):
        c = int(model.t_chunk_enc if t_chunk_enc is None else t_chunk_enc)
        check_sessions_supported(model)
        f = model.encoder.time_downsample_factor
        if c < 1 or c % f:
            raise ValueError(f"EncodeSession: t_chunk_enc ({c}) must be a positive multiple of the temporal factor {f}")
        super().__init__(model, model.encoder, c, 0)
        self.t_chunk_enc = c
        self.chunk_losses = []

    def _alloc_pending(self):
        B, C, H, W = self._geom
        self._pend = torch.empty((B, C, self.sched.step, H, W), dtype=torch.float32, device=self._device)

    def _run(self, src, t0, t1, first, look):
        m = self.model
        chunk_z = super()._run(src, t0, t1, first, look)
        return m.regularization(chunk_z, n_steps=m.global_step // 2)

    def _collect(self, outs):
        logs = [lg for _, lg in outs]
        for lg in logs:
            self._loss_key = "kl_loss" if "kl_loss" in lg else "aux_loss"
            self.chunk_losses.append(lg[self._loss_key])
        if outs and self._out_shape is None:
            z0, lg0 = outs[0]
            self._out_shape = (z0.shape[0], z0.shape[1]) + tuple(z0.shape[3:])
            self._idx_tail = tuple(lg0["indices"].shape[2:]) if "indices" in lg0 else None
        B, Cz, h, w = self._out_shape
        n = sum(z.shape[2] for z, _ in outs)
        z = torch.empty((B, Cz, n, h, w), dtype=torch.float32, device=self._device)
        idx = None if self._idx_tail is None else torch.empty((B, n) + self._idx_tail, dtype=torch.int32, device=self._device)
        done = 0
        for cz, lg in outs:
            k = cz.shape[2]
            ops.ncthw_copy_frames(cz.contiguous(), z, 0, done, k)
            if idx is not None:
                ops.gather_frames(lg["indices"].contiguous(), list(range(k)), out=idx, out_t0=done)
            done += k
        log = {"chunk_logs": logs}
        if idx is not None:
            log["indices"] = idx
        return z, log

    @torch.no_grad()
    def push(self, x):
        """x: fp32 NCTHW frames on the GPU, n >= 1 of them"""
        self._check_input(x, "EncodeSession.push")
        if self.sched.finished:
            raise RuntimeError("EncodeSession.push: the session is finished")
        self._device = x.device
        self._sync_mode(x)
        x = x.contiguous().float()
        outs = self._advance(x.shape[2], lambda dst, d0, s0, k: ops.ncthw_copy_frames(x, dst, s0, d0, k), direct=x)
        return self._collect(outs)

    @torch.no_grad()
    def push_u8(self, frames_u8, input_height, input_width):
        """decoded video frames uint8 [n, H0, W0, 3] on the GPU (B = 1): resized, cropped and normalised straight into the
        session's chunk buffer (video_io.preprocess_frames: vt_frames_u8_to_ncthw), never as one fp32 tensor"""
        from .video_io import preprocess_frames

        if not (isinstance(frames_u8, torch.Tensor) and frames_u8.is_cuda and frames_u8.dtype == torch.uint8 and frames_u8.dim() == 4):
            raise ValueError("EncodeSession.push_u8: uint8 [n, H0, W0, 3] frames on the GPU")
        geom = (1, 3, int(input_height), int(input_width))
        if self._geom is None:
            self._geom = geom
        elif geom != self._geom:
            raise ValueError(f"EncodeSession.push_u8: B / C / H / W {geom} differ from the first push's {self._geom}")
        if self.sched.finished:
            raise RuntimeError("EncodeSession.push_u8: the session is finished")
        self._device = frames_u8.device
        self._sync_mode(frames_u8)

        def fill(dst, d0, s0, k):
            preprocess_frames(frames_u8[s0:s0 + k], input_height, input_width, out=dst, t_off=d0)

        return self._collect(self._advance(frames_u8.shape[0], fill))

    @torch.no_grad()
    def finish(self):
        if self._geom is None:
            raise RuntimeError("EncodeSession.finish: nothing was pushed")
        self._sync_mode(self._pend)
        return self._collect(self._advance(None, None))

    def reg_log(self):
        """the mean of the per-chunk losses, as tile_encode reports it"""
        if not self.chunk_losses:
            raise RuntimeError("EncodeSession.reg_log: no chunk has run yet")
        return {self._loss_key: torch.mean(torch.stack(self.chunk_losses))}


class DecodeSession(_Session):
    """push(z) / finish() -> fp32 frames [B, out_ch, n, H, W] of the chunks the call completed (n may be 0).  Input: latents fp32
    [B, C, n', H', W'], or FSQ indices int32 [B, n', H', W'] with from_indices=True (indices_to_latent per push)."""

    _graphed_name = "_gdec"

    def __init__(self, model, t_chunk_dec=None, use_overlap=None, from_indices=False):
        check_sessions_supported(model)
        c = int(model.t_chunk_dec if t_chunk_dec is None else t_chunk_dec)
        if c < 1:
            raise ValueError(f"DecodeSession: t_chunk_dec must be >= 1 (got {c})")
        self.use_overlap = bool(model.use_overlap if use_overlap is None else use_overlap)
        super().__init__(model, model.decoder, c, 1 if self.use_overlap else 0)
        self.t_chunk_dec, self.from_indices = c, bool(from_indices)
        self.frames_out = 0

    def _alloc_pending(self):
        B, C, H, W = self._geom
        self._pend = torch.empty((B, C, self.sched.step + self.sched.lookahead, H, W), dtype=torch.float32, device=self._device)

    def _run(self, src, t0, t1, first, look):
        chunk = super()._run(src, t0, t1, first, look)
        n = chunk.shape[2] - (self.f if look else 0)
        dst = self._out
        ops.ncthw_copy_frames(chunk.contiguous(), dst, 0, self._done, n)   # now: a replayed chunk's output is the graph's own buffer
        self._done += n
        return n

    def _empty_out(self, n):
        B, _, H, W = self._geom
        s = 2 ** len(self.model.decoder.spatial_us)
        return torch.empty((B, self.model.decoder.out_ch, n, H * s, W * s), dtype=torch.float32, device=self._device)

    def _step(self, n, z=None):
        # the frames this call emits are known before anything runs: one output tensor, filled chunk by chunk
        probe = ChunkSchedule(self.sched.step, self.sched.lookahead)
        probe.received, probe.start, probe.index, probe.finished = self.sched.received, self.sched.start, self.sched.index, False
        total = decode_emission(probe.push(n) if n is not None else probe.finish(), self.f)
        self._out, self._done = self._empty_out(total), 0
        fill = None if z is None else (lambda dst, d0, s0, k: ops.ncthw_copy_frames(z, dst, s0, d0, k))
        self._advance(n, fill, direct=z)
        assert self._done == total, (self._done, total)
        out, self._out = self._out, None
        self.frames_out += total
        return out

    @torch.no_grad()
    def push(self, z):
        if self.from_indices:
            if not (isinstance(z, torch.Tensor) and z.is_cuda and z.dim() >= 4):
                raise ValueError("DecodeSession.push: FSQ indices [B, n, H', W'] on the GPU")
            z = self.model.tile_indices_to_latent(z)
        self._check_input(z, "DecodeSession.push")
        if self.sched.finished:
            raise RuntimeError("DecodeSession.push: the session is finished")
        self._device = z.device
        self._sync_mode(z)
        z = z.contiguous().float()
        return self._step(z.shape[2], z)

    @torch.no_grad()
    def finish(self):
        if self._geom is None:
            raise RuntimeError("DecodeSession.finish: nothing was pushed")
        self._sync_mode(self._pend)
        return self._step(None)


class ReconstructSession:
    """encode session -> regularizer -> decode session: emits exactly tile_decode(tile_encode(x)), in order.  forward() keeps
    the last T of those frames; how many leading frames it drops depends on the last chunk's front padding, so finish() returns
    (frames, drop) with `drop` counted from the first frame the session emitted."""

    def __init__(self, model, t_chunk_enc=None, t_chunk_dec=None, use_overlap=None):
        check_sessions_supported(model)
        c = int(model.t_chunk_enc if t_chunk_enc is None else t_chunk_enc)
        self.enc = EncodeSession(model, c)
        self.dec = DecodeSession(model, model.t_chunk_dec if t_chunk_dec is None else t_chunk_dec, use_overlap)
        self.frames_in = 0
        self.last_log = None

    def _through(self, z_log):
        z, self.last_log = z_log
        if z.shape[2] == 0:
            return self.dec._empty_out(0) if self.dec._geom is not None else None
        return self.dec.push(z)

    @torch.no_grad()
    def push(self, x):
        out = self._through(self.enc.push(x))
        self.frames_in += x.shape[2]
        return out

    @torch.no_grad()
    def push_u8(self, frames_u8, input_height, input_width):
        out = self._through(self.enc.push_u8(frames_u8, input_height, input_width))
        self.frames_in += frames_u8.shape[0]
        return out

    @torch.no_grad()
    def finish(self):
        a = self._through(self.enc.finish())
        b = self.dec.finish()
        out = b if a is None or a.shape[2] == 0 else (a if b.shape[2] == 0 else _cat_frames(a, b))
        return out, self.dec.frames_out - self.frames_in


def _cat_frames(a, b):
    out = torch.empty(tuple(a.shape[:2]) + (a.shape[2] + b.shape[2],) + tuple(a.shape[3:]), dtype=a.dtype, device=a.device)
    ops.ncthw_copy_frames(a, out, 0, 0, a.shape[2])
    ops.ncthw_copy_frames(b, out, 0, a.shape[2], b.shape[2])
    return out
