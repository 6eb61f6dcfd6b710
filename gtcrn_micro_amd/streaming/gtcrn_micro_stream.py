"""Host-side mirror of ``gtcrn_micro.streaming.gtcrn_micro_stream.StreamGTCRNMicro``.

``forward(spec, conv_cache, tra_cache, tcn_cache)`` keeps the reference call
(gtcrn_micro_stream.py:541-574): the caller owns the three caches in the reference
shapes -- conv_cache (2,B,16,6,33), tra_cache (2,3,B,8,2), tcn_cache 2 x 4 tensors
(B,16,2d,33) (:618-623) -- and gets them back updated (in place, like the reference).

Internally the HIP kernels keep per-stream ring state on the device.  The reference loop
(:626-635) passes the returned caches straight back in, frame after frame, and never looks
inside them; converting caches -> rings -> caches on every frame would cost two extra
kernels per 16 ms frame for nothing.  So:

* **import is skipped** when the caches received are the ones returned by the previous call
  and nobody wrote to them since (object identity + the tensors' version counters);
* **export is lazy**: the returned caches are thin ``torch.Tensor`` subclasses over the
  caller's own storage whose contents are brought up to date the moment anything READS
  or WRITES them (any torch operation on them: indexing, ``.cpu()``, ``torch.equal``,
  in-place edits, printing, ``data_ptr()`` / ``__dlpack__`` / ``__cuda_array_interface__`` ...),
  or explicitly with ``sync_caches()`` -- REQUIRED before a raw pointer obtained EARLIER (or
  from the caller's original tensor objects) is read by foreign code.  A caller that
  keeps using its ORIGINAL tensor objects instead of the returned ones (legal: the
  reference mutates them in place) cannot be intercepted, so for that call pattern the
  export runs eagerly every frame (import is still skipped while they stay untouched).

``init_state`` / ``step`` is the native form that leaves the state on the device; ``init_wave_state`` /
``step_wave`` / ``flush_wave`` the same at the waveform: 256 samples (one hop) in, 256 enhanced out, one hop late
(include/gtcrn_micro_hip.h, gtcrn_wave_stream_*).
"""
import torch

from .. import _lib
from ..models.gtcrn_micro import GTCRNMicro

# metadata a caller (or this module) may ask of a lazy cache without needing its contents.  NOT in the list, on
# purpose: everything that hands out the memory itself -- ``data_ptr``, ``untyped_storage``, ``__cuda_array_interface__``,
# ``__dlpack__`` -- so a caller that passes a returned cache's raw pointer to its own kernels reads current data.
_META = {"shape", "dtype", "device", "layout", "requires_grad", "is_cuda", "ndim", "_version", "grad", "grad_fn",
         "is_leaf", "names", "is_sparse", "is_quantized", "is_meta", "size", "dim", "stride", "numel",
         "is_contiguous", "storage_offset", "element_size", "nelement", "ndimension", "get_device", "__len__",
         "is_inference"}


class _LazyCache(torch.Tensor):
    """A cache tensor handed back by ``StreamGTCRNMicro.forward``: same storage as the caller's tensor, brought up to
    date from the device ring state before the first operation that touches its contents."""

    @staticmethod
    def wrap(t, owner):
        w = torch.Tensor._make_subclass(_LazyCache, t, False)
        w._owner = owner
        return w

    def __deepcopy__(self, memo):
        """``copy.deepcopy`` of a returned cache: an ordinary tensor holding the current contents."""
        owner = getattr(self, "_owner", None)
        if owner is not None:
            owner.sync_caches()
        with torch._C.DisableTorchFunctionSubclass():
            return self.as_subclass(torch.Tensor).clone()

    def _current(self):
        owner = getattr(self, "_owner", None)
        if owner is not None:
            owner.sync_caches()
        with torch._C.DisableTorchFunctionSubclass():
            return self.as_subclass(torch.Tensor)

    # the zero-copy export protocols, spelled out (they hand the memory to foreign code)
    def __dlpack__(self, *args, **kwargs):
        return self._current().__dlpack__(*args, **kwargs)

    @property
    def __cuda_array_interface__(self):
        return self._current().__cuda_array_interface__

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = getattr(func, "__name__", "")
        if name == "__get__":                                      # property getter: func.__self__ is the descriptor
            name = getattr(getattr(func, "__self__", None), "__name__", "")
        if name not in _META:
            for a in args:
                owner = getattr(a, "_owner", None) if isinstance(a, _LazyCache) else None
                if owner is not None:
                    owner.sync_caches()
        with torch._C.DisableTorchFunctionSubclass():
            return func(*args, **kwargs)


class StreamGTCRNMicro(GTCRNMicro):
    """Streaming twin: same parameters as the offline model (``convert_to_stream`` copies them)."""

    def __init__(self, n_fft=512, hop_len=256, win_len=512):
        super().__init__(n_fft, hop_len, win_len)
        self._scratch = {}
        self._bound = None          # the caches handed out by the previous call (see forward)
        self.forward_stats = {"calls": 0, "imports": 0, "exports": 0}

    @staticmethod
    def init_caches(batch, device):
        """Zero caches in the reference layout (gtcrn_micro_stream.py:618-623)."""
        conv_cache = torch.zeros(2, batch, 16, 6, 33, device=device)
        tra_cache = torch.zeros(2, 3, batch, 8, 2, device=device)
        tcn_cache = [[torch.zeros(batch, 16, 2 * d, 33, device=device) for d in (1, 2, 4, 8)] for _ in range(2)]
        return conv_cache, tra_cache, tcn_cache

    # ---- the cache <-> ring-state binding ----------------------------------------------------------
    def _match(self, flat):
        """0: unrelated caches (import needed); 1: exactly the lazy caches handed out last call, untouched;
        2: the caller's own original tensors of last call, untouched."""
        bd = self._bound
        if bd is None:
            return 0
        with torch._C.DisableTorchFunctionSubclass():
            if all(a is b for a, b in zip(flat, bd["lazy"])):
                kind = 1
            elif all(a is b for a, b in zip(flat, bd["orig"])):
                kind = 2
            else:
                return 0
            # in-place writes by the caller (through either object: they share the version counter) invalidate it
            if any(t._version != v for t, v in zip(bd["orig"], bd["versions"])):
                return 0
        return kind

    def sync_caches(self):
        """Brings the caches handed out by the last ``forward`` up to date with the device ring state (no-op if they
        already are).  Called automatically when a lazy cache is read or written."""
        bd = self._bound
        if bd is None or not bd["pending"]:
            return
        bd["pending"] = False
        with torch._C.DisableTorchFunctionSubclass():
            conv, tra = bd["orig"][0], bd["orig"][1]
            tcn = [bd["orig"][2:6], bd["orig"][6:10]]
            bd["eng"].stream_export(bd["state"], conv, tra, tcn)
            bd["versions"] = [t._version for t in bd["orig"]]     # our own write is not a caller's edit
        self.forward_stats["exports"] += 1

    def forward(self, spec, conv_cache, tra_cache, tcn_cache):
        if self.training:
            raise NotImplementedError("streaming inference is eval-mode only; call .eval()")
        if not spec.is_cuda:
            raise _lib.GtcrnError("StreamGTCRNMicro.forward needs CUDA (ROCm) tensors: there is no CPU path")
        B = spec.shape[0]
        with torch._C.DisableTorchFunctionSubclass():
            if tuple(conv_cache.shape) != (2, B, 16, 6, 33):
                raise AssertionError(f"conv_cache must be (2,{B},16,6,33), got {tuple(conv_cache.shape)}")
            if tuple(tra_cache.shape) != (2, 3, B, 8, 2):
                raise AssertionError(f"tra_cache must be (2,3,{B},8,2), got {tuple(tra_cache.shape)}")
            for g in range(2):
                for k, d in enumerate((1, 2, 4, 8)):
                    if tuple(tcn_cache[g][k].shape) != (B, 16, 2 * d, 33):
                        raise AssertionError(f"tcn_cache[{g}][{k}] must be ({B},16,{2 * d},33)")
        eng = self.engine(spec.device)
        flat = [conv_cache, tra_cache] + [tcn_cache[g][k] for g in range(2) for k in range(4)]
        self.forward_stats["calls"] += 1
        with torch._C.DisableTorchFunctionSubclass():
            untracked = any(t.is_inference() for t in flat)
        if untracked:
            # Caches created under torch.inference_mode() (infer.py runs in it) carry no version counter, so a caller's
            # edit between two calls could not be seen: such caches take the plain route every frame -- import, step,
            # export into the caller's own tensors, which are returned as they are (the reference's in-place contract).
            return self._forward_eager(eng, spec, B, flat, conv_cache, tra_cache, tcn_cache)
        kind = self._match(flat)
        if kind and (self._bound["eng"] is not eng or self._bound["B"] != B):
            kind = 0
        if kind == 0:
            # unknown or modified caches: whatever an earlier binding still owes its caller is written out first -- this
            # module's own, and the binding of ANY OTHER StreamGTCRNMicro that handed these caches out (an A/B of two
            # models, a hot swap via convert_to_stream mid-stream: their pending export is this call's input) -- then
            # the ring state is rebuilt from the caches received
            self.sync_caches()
            for t in flat:
                owner = getattr(t, "_owner", None) if isinstance(t, _LazyCache) else None
                if owner is not None and owner is not self:
                    owner.sync_caches()
            key = (spec.device.index, B)
            state = self._scratch.get(key)
            if state is None:
                state = eng.new_state(B)
                self._scratch[key] = state
            with torch._C.DisableTorchFunctionSubclass():
                orig = [t.as_subclass(torch.Tensor) if isinstance(t, _LazyCache) else t for t in flat]
                eng.stream_import(state, orig[0], orig[1], [orig[2:6], orig[6:10]])
            self.forward_stats["imports"] += 1
            lazy = [_LazyCache.wrap(t, self) for t in orig]
            self._bound = {"eng": eng, "B": B, "state": state, "orig": orig, "lazy": lazy, "pending": False,
                           "versions": None}
        bd = self._bound
        out = eng.stream_step(bd["state"], spec)
        bd["pending"] = True
        with torch._C.DisableTorchFunctionSubclass():
            bd["versions"] = [t._version for t in bd["orig"]]
        if kind != 1:
            # the caller holds plain tensors whose reads cannot be intercepted (its own originals, or a fresh binding
            # whose caller may go either way): keep them current.  Only a caller that passes the RETURNED caches back
            # gets the deferred export.
            self.sync_caches()
        if kind == 2:
            return out, conv_cache, tra_cache, tcn_cache
        lz = bd["lazy"]
        return out, lz[0], lz[1], [lz[2:6], lz[6:10]]

    def _forward_eager(self, eng, spec, B, flat, conv_cache, tra_cache, tcn_cache):
        """import -> step -> export on every call: for caches whose edits cannot be tracked (inference tensors)."""
        self.sync_caches()                                   # an earlier (tracked) binding may still owe an export
        self._bound = None
        key = (spec.device.index, B)
        state = self._scratch.get(key)
        if state is None:
            state = eng.new_state(B)
            self._scratch[key] = state
        eng.stream_import(state, flat[0], flat[1], [flat[2:6], flat[6:10]])
        self.forward_stats["imports"] += 1
        out = eng.stream_step(state, spec)
        eng.stream_export(state, flat[0], flat[1], [flat[2:6], flat[6:10]])
        self.forward_stats["exports"] += 1
        return out, conv_cache, tra_cache, tcn_cache

    # ---- native streaming: state stays in the library's ring layout on the device ---------------
    def init_state(self, nstreams, device="cuda"):
        dev = torch.device(device)
        return self.engine(dev).new_state(nstreams)

    def step(self, spec_t, state):
        """spec_t (N,257,n,2), n >= 1 new frames per stream; state from init_state (updated in place)."""
        return self.engine(spec_t.device).stream_step(state, spec_t)

    def init_wave_state(self, nstreams, window, device="cuda", fs=16000, packet=None, atten_lim_db=None, state=None, slots=None,
                        count=None, resident=False, max_active=None, meters=False, g711=None, highband=None, ramp=False,
                        alc=None, tones=None):
        """State of `nstreams` waveform streams (Engine.new_wave_state); window: the 512-tap analysis / synthesis window
        of the offline call, window[0] == 0 (torch.hann_window(512).pow(0.5) for infer.py's).  fs: the caller's sample
        rate; 8000, 24000, 32000 or 48000 gives the rate form (Engine.new_rate_state: hops of 256 fs / 16000 samples).
        packet: the caller's block size in samples at fs (e.g. 160 = 10 ms at 16 kHz, 441 at 44.1 kHz) gives the packet
        form (Engine.new_packet_state: one packet in, one out per call, at 8 / 16 / 22.05 / 24 / 32 / 44.1 / 48 kHz).
        atten_lim_db: the attenuation limit in dB, one value or one per stream (None: off; 0: bypass at the form's
        latency); state.set_atten_lim_db changes it while the streams run.
        meters=True: the state owns per-stream level meters (state.meters, state.levels(), state.reset_meters()) that every
        step and flush of it updates.
        ramp=True: the state owns state.gain_ramp, and a later state.set_atten_lim_db is spread over the next emitted block
        (16 ms at 16 kHz) instead of landing as a step; set_atten_lim_db(..., snap=True) changes at once.
        alc= ("vad": the voice flag only; True: the default level control; a mapping of its settings): the state owns
        state.alc and state.alc_params -- a speech-gated output gain, a limiter and state.voice() per stream, made at 16 kHz
        in every step and flush (state.set_alc, state.alc_gain_db(), state.reset_alc()); not together with highband=.
        tones= ("detect": the detector only; True: the default tone guard; a mapping of its settings): the state owns
        state.tones -- DTMF digits, 1100 Hz and 2100 Hz are detected per stream at 16 kHz in every step and flush
        (state.tone(), state.tone_events()) and, unless "detect", the blocks that hold one are passed dry (state.set_tones,
        state.reset_tones()).
        state=, slots= (int32 device tensor), count= (device int32, optional): a stream JOINS -- the named slots of the
        existing 16 kHz `state` are reset to the start of a clip (Engine.wave_stream_reset_slots, a capturable kernel) and
        `state` is returned; the other slots are not touched.  Rate states and plain packet states cannot be addressed by
        slot (their streams share a group phase).
        packet=, resident=True: `nstreams` RESIDENT packet streams with a phase each (Engine.new_packet_slot_state; at most
        `max_active`, default all, step per call); state=<that state>, slots= resets its named slots
        (Engine.packet_stream_reset_slots).
        g711="ulaw" | "alaw" (with packet=): step_wave then also takes and returns torch.uint8 rows of G.711 codes of that
        law (fs=8000, packet=160, g711="ulaw": 20 ms PCMU packets); float32 and int16 rows stay legal.
        highband= (with fs = 24000, 32000 or 48000): the gain, one value or one per stream (slot) in [0, 1], with which the
        band above 8 kHz is carried around the model (state.set_highband_gain changes it while the streams run): the rate
        form without packet= (Engine.new_rate_state), the packet form and the resident packet slots with it
        (Engine.new_packet_state / new_packet_slot_state; not with g711=).  None: that band is not in the output."""
        if _lib._alc_on(alc) and slots is not None:
            raise _lib.GtcrnError("alc= is given when a state is made, not when slots= resets some of its streams")
        if _lib._tones_on(tones) and slots is not None:
            raise _lib.GtcrnError("tones= is given when a state is made, not when slots= resets some of its streams")
        if highband is not None and slots is not None:
            raise _lib.GtcrnError("highband= is given when a state is made, not when slots= resets some of its streams")
        if g711 is not None and (packet is None or slots is not None):
            raise _lib.GtcrnError("g711= goes with packet=: G.711 codes are taken by the packet forms only")
        eng = self.engine(torch.device(device))
        if slots is not None:
            if isinstance(state, _lib.PacketSlotState):
                eng.packet_stream_reset_slots(state, slots, count=count)
                return state
            if state is None or packet is not None or int(fs) != 16000:
                raise _lib.GtcrnError("slots= resets slots of an existing 16 kHz wave state: pass state=, no fs / packet")
            eng.wave_stream_reset_slots(state, slots, count=count)
            return state
        if resident:
            if packet is None:
                raise _lib.GtcrnError("resident=True makes a packet slot state: pass packet= (a 16 kHz wave state is resident as it is)")
            return eng.new_packet_slot_state(nstreams, window, int(packet), int(fs), max_active=max_active,
                                             atten_lim_db=atten_lim_db, meters=meters, g711=g711, highband=highband, ramp=ramp, alc=alc, tones=tones)
        if packet is not None:
            return eng.new_packet_state(nstreams, window, int(packet), int(fs), atten_lim_db=atten_lim_db, meters=meters,
                                        g711=g711, highband=highband, ramp=ramp, alc=alc, tones=tones)
        if int(fs) != 16000:
            return eng.new_rate_state(nstreams, window, int(fs), atten_lim_db=atten_lim_db, meters=meters, highband=highband, ramp=ramp,
                                      alc=alc, tones=tones)
        if highband is not None:
            raise _lib.GtcrnError("highband= needs fs = 24000, 32000 or 48000: a 16 kHz stream has no band above 8 kHz")
        return eng.new_wave_state(nstreams, window, atten_lim_db=atten_lim_db, meters=meters, ramp=ramp, alc=alc, tones=tones)

    def step_wave(self, x, state, slots=None, count=None):
        """x (N, 256*n) float32 or int16, n >= 1 hops per stream -> the enhanced hops, same dtype, one hop late.  With a
        state made for another rate: hops of state.hop samples at that rate, state.latency samples late.  With a packet
        state: exactly one packet of state.packet samples per stream, state.latency16 samples (at 16 kHz) late; made with
        g711=, it also takes torch.uint8 rows of G.711 codes and returns codes.
        slots= (int32 device tensor, M ids), count= (device int32, optional): the live tick of a server -- x (M, 256), row i
        is the stream in slot slots[i] of the 16 kHz `state`, `count` rows step, no other slot is touched
        (Engine.wave_stream_step_slots).  With a packet slot state (init_wave_state(..., packet=, resident=True)): x
        (M, state.packet), one packet per named slot (Engine.packet_stream_step_slots).  Rate states and plain packet
        states raise: their streams share a group phase."""
        if slots is not None:
            if isinstance(state, _lib.PacketSlotState):
                return self.engine(x.device).packet_stream_step_slots(state, slots, x, count=count)
            return self.engine(x.device).wave_stream_step_slots(state, slots, x, count=count)
        if isinstance(state, _lib.PacketStreamState):
            return self.engine(x.device).packet_stream_step(state, x)
        if isinstance(state, _lib.RateStreamState):
            return self.engine(x.device).rate_stream_step(state, x)
        return self.engine(x.device).wave_stream_step(state, x)

    def flush_wave(self, tail, state, slots=None, count=None):
        """tail (N, r), r = 0..255 samples after the last whole hop -> the last 256 enhanced samples per stream.
        slots=, count=: the named streams of a 16 kHz state leave (Engine.wave_stream_flush_slots); tail is (M, r)."""
        if slots is not None:
            return self.engine(tail.device).wave_stream_flush_slots(state, slots, tail, count=count)
        return self.engine(tail.device).wave_stream_flush(state, tail)
