"""Packet loss concealment (include/gtcrn_micro_hip.h, "packet loss concealment"): a lost packet's row
is filled with the pitch-synchronous continuation of the stream's history, held, faded out, and cross-faded back into the
real signal, on the device where the live step is about to read the rows.  `Concealer` owns the histories, records and
parameter words of the streams on one device; `plc_params` and `plc_rows_host` are the host side of the same contract (the
parameter words, and the functions the kernel compiles run on numpy arrays)."""
import ctypes

import numpy as np

from ._lib import GtcrnError, _check, _stream_ptr, g711_law, lib

PLC_DEFAULTS = {"hold_ms": 10, "fade_ms": 50, "recover_ms": 5}
PLC_RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
PLC_MAX_N = 1024


class PlcConfig(ctypes.Structure):
    _fields_ = [("fs", ctypes.c_int), ("hold_ms", ctypes.c_int), ("fade_ms", ctypes.c_int), ("recover_ms", ctypes.c_int)]


def _whole(name, v):
    if isinstance(v, bool) or (isinstance(v, float) and not v.is_integer()):
        raise GtcrnError(f"{name} must be a whole number, got {v!r}")
    try:
        return max(min(int(v), 1 << 30), -(1 << 30))
    except (OverflowError, ValueError, TypeError):
        raise GtcrnError(f"{name} must be a whole number, got {v!r}") from None


def plc_params(fs, **fields):
    """The 8 parameter words {pmin, pmax, W, D, T0, T1, F, fs} of the concealment at rate `fs` for the defaults (hold_ms=10,
    fade_ms=50, recover_ms=5) with `fields` replaced: an int32 array from gtcrn_plc_params_host, the one place they are made."""
    unknown = set(fields) - set(PLC_DEFAULTS)
    if unknown:
        raise GtcrnError(f"unknown concealment fields {sorted(unknown)}: the config has {sorted(PLC_DEFAULTS)}")
    f = dict(PLC_DEFAULTS, **fields)
    cfg = PlcConfig(_whole("fs", fs), _whole("hold_ms", f["hold_ms"]), _whole("fade_ms", f["fade_ms"]), _whole("recover_ms", f["recover_ms"]))
    out = np.empty(8, np.int32)
    _check(lib().gtcrn_plc_params_host(ctypes.byref(cfg), out.ctypes.data))
    return out


def plc_history_len(params):
    """Lh = pmax + W of a block of parameter words."""
    return int(params[1]) + int(params[2])


def _aligned(n, dtype):
    """A zeroed array of n elements whose first byte is 16-byte aligned."""
    item = np.dtype(dtype).itemsize
    raw = np.zeros(n * item + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n * item].view(dtype)


_KINDS = {np.dtype(np.float32): "gtcrn_plc_rows", np.dtype(np.int16): "gtcrn_plc_rows_pcm16", np.dtype(np.uint8): "gtcrn_plc_rows_g711"}


def plc_rows_host(x, lost, hist, rec, params, slots=None, count=None, g711=None):
    """gtcrn_plc_rows_host / _pcm16_host / _g711_host on numpy arrays: x (M, n) float32, int16 or uint8 codes (rows may be a strided
    view), hist (S, >= Lh) int16 and rec (S, 4) int32 are written in place; lost (M,) and slots (M,) or None int32; params the 8
    words; count None or a number; g711 the law of uint8 rows."""
    if x.dtype not in _KINDS or x.ndim != 2:
        raise GtcrnError("x must be a (rows, n) array of float32, int16 or uint8")
    item = x.dtype.itemsize
    n = x.shape[1]
    if (n > 1 and x.strides[1] != item) or x.strides[0] % item or not x.flags.writeable:
        raise GtcrnError("the samples of a row must be contiguous and writeable")
    law = g711_law(g711)
    if x.dtype == np.uint8 and law is None:
        raise GtcrnError('x is uint8 (G.711 codes): pass g711="ulaw" or "alaw"')
    if hist.dtype != np.int16 or hist.ndim != 2 or (hist.shape[1] > 1 and hist.strides[1] != 2) or hist.strides[0] % 2:
        raise GtcrnError("hist must be an (S, Lh) int16 array with contiguous rows")
    if rec.dtype != np.int32 or rec.ndim != 2 or rec.shape[1] != 4 or rec.shape[0] != hist.shape[0] or not rec.flags.c_contiguous:
        raise GtcrnError("rec must be a contiguous (S, 4) int32 array, a record per history")
    los = np.ascontiguousarray(lost, np.int32).reshape(-1)
    if los.size != x.shape[0]:
        raise GtcrnError("lost must hold a word per row")
    ids = None if slots is None else np.ascontiguousarray(slots, np.int32).reshape(-1)
    if ids is not None and ids.size != x.shape[0]:
        raise GtcrnError("slots must hold an id per row")
    words = _aligned(8, np.int32)
    words[:] = np.asarray(params, np.int32)
    records = _aligned(rec.size, np.int32)
    records[:] = rec.reshape(-1)
    cnt = None if count is None else np.array([count], np.int32)
    args = [x.ctypes.data, max(x.strides[0] // item, n) if x.shape[0] > 1 else n, x.shape[0], n, None if ids is None else ids.ctypes.data,
            los.ctypes.data, None if cnt is None else cnt.ctypes.data, hist.ctypes.data,
            max(hist.strides[0] // 2, 1) if hist.shape[0] > 1 else max(hist.shape[1], 1), records.ctypes.data, hist.shape[0], words.ctypes.data]
    if x.dtype == np.uint8:
        args.append(law)
    _check(getattr(lib(), _KINDS[x.dtype] + "_host")(*args))
    rec[:] = records.reshape(rec.shape)


class Concealer:
    """The concealment state of `streams` streams on one device: histories (streams, Lh) int16, records (streams, 4) int32 and
    the parameter words, all of fixed address, so that a captured graph that holds a `conceal` call stays valid while the
    loss flags, the slots, the row count and the parameters change between replays."""

    def __init__(self, streams, fs, n, device, dtype, g711=None, hold_ms=10, fade_ms=50, recover_ms=5):
        import torch
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.type != "cuda":
            raise GtcrnError("a Concealer lives on a CUDA (ROCm) device: there is no CPU path")
        self.streams, self.fs, self.n = int(streams), int(fs), int(n)
        if self.streams < 1:
            raise GtcrnError("streams must be positive")
        if not 1 <= self.n <= PLC_MAX_N:
            raise GtcrnError(f"n must lie in 1 .. {PLC_MAX_N}, got {n}")
        if dtype not in (torch.float32, torch.int16, torch.uint8):
            raise GtcrnError("dtype must be torch.float32, torch.int16 or torch.uint8 (G.711 codes)")
        self.dtype, self.g711 = dtype, g711_law(g711)
        if dtype == torch.uint8 and self.g711 is None:
            raise GtcrnError('uint8 rows are G.711 codes: pass g711="ulaw" or "alaw"')
        if dtype != torch.uint8 and self.g711 is not None:
            raise GtcrnError("g711= goes with dtype=torch.uint8")
        self.fields = dict(PLC_DEFAULTS)
        words = plc_params(self.fs, hold_ms=hold_ms, fade_ms=fade_ms, recover_ms=recover_ms)
        self.history_len = plc_history_len(words)
        z = lambda shape, dt: torch.zeros(shape, device=self.device, dtype=dt)
        self.hist = z((self.streams, self.history_len), torch.int16)
        self.rec = z((self.streams, 4), torch.int32)
        self.params = z((8,), torch.int32)
        self.set_params(hold_ms=hold_ms, fade_ms=fade_ms, recover_ms=recover_ms)

    def set_params(self, **fields):
        """Replaces the named fields (hold_ms, fade_ms, recover_ms) and writes the parameter words in place."""
        import torch
        words = plc_params(self.fs, **dict(self.fields, **fields))
        self.fields.update(fields)
        self.params.copy_(torch.from_numpy(words).pin_memory(), non_blocking=True)

    def _table(self, t, what, rows):
        import torch
        if t is None:
            return None
        if not isinstance(t, torch.Tensor):
            ids = [int(v) for v in t]
            if what == "slots":
                if len(set(ids)) != len(ids):
                    raise GtcrnError("slots names a stream twice")
                if any(not 0 <= v < self.streams for v in ids):
                    raise GtcrnError(f"slots must lie in 0 .. {self.streams - 1}")
            t = torch.tensor(ids, dtype=torch.int32, device=self.device)
        if t.device != self.device or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or (rows is not None and t.shape[0] < rows):
            raise GtcrnError(f"{what} must be a contiguous 1-D int32 tensor on {self.device}" + (f" of at least {rows} words" if rows else ""))
        return t

    def _count(self, count):
        import torch
        if count is None or isinstance(count, torch.Tensor):
            if count is not None and (count.device != self.device or count.dtype != torch.int32 or count.numel() < 1):
                raise GtcrnError(f"count must be an int32 tensor on {self.device}")
            return count
        return torch.tensor([int(count)], dtype=torch.int32, device=self.device)

    def conceal(self, x, lost, slots=None, count=None):
        """One tick, in place: x (M, n) on the device, the rows the step is about to take; lost (M,) int32, non-zero where the
        packet did not arrive (a sequence is uploaded); slots (M,) int32 names the stream of each row (None: row i is stream
        i; a host sequence is checked for duplicates); count: an int32 device word, rows at or beyond it are skipped.  One
        launch, asynchronous, capturable when lost, slots and count are device tensors.  Returns x."""
        import torch
        if not isinstance(x, torch.Tensor) or x.device != self.device or x.dim() != 2:
            raise GtcrnError(f"x must be a (rows, n) tensor on {self.device}")
        if x.dtype != self.dtype:
            raise GtcrnError(f"x is {x.dtype} but the state was made for {self.dtype}")
        M, n = x.shape
        if n != self.n:
            raise GtcrnError(f"x has rows of {n} samples but the state was made for n = {self.n}")
        if n > 1 and x.stride(1) != 1:
            raise GtcrnError("the samples of a row must be contiguous")
        if slots is None and M > self.streams:
            raise GtcrnError(f"x has {M} rows but the state holds {self.streams} streams")
        lost = self._table(lost, "lost", M)
        slots = self._table(slots, "slots", M)
        count = self._count(count)
        args = [x.data_ptr(), max(x.stride(0), n) if M > 1 else n, M, n, None if slots is None else slots.data_ptr(), lost.data_ptr(),
                None if count is None else count.data_ptr(), self.hist.data_ptr(), self.history_len, self.rec.data_ptr(), self.streams,
                self.params.data_ptr()]
        if self.dtype == torch.uint8:
            args.append(self.g711)
        with torch.cuda.device(self.device):
            name = {torch.float32: "gtcrn_plc_rows", torch.int16: "gtcrn_plc_rows_pcm16", torch.uint8: "gtcrn_plc_rows_g711"}[self.dtype]
            _check(getattr(lib(), name)(*args, _stream_ptr()))
        return x

    def reset(self, slots=None, count=None):
        """Zeroes the histories and records of `slots` (None: every stream) below `count`: fresh streams.  One launch of its own,
        asynchronous and capturable like conceal."""
        import torch
        slots = self._table(slots, "slots", None)
        M = self.streams if slots is None else slots.shape[0]
        count = self._count(count)
        with torch.cuda.device(self.device):
            _check(lib().gtcrn_plc_reset(self.hist.data_ptr(), self.history_len, self.rec.data_ptr(), self.streams, self.params.data_ptr(),
                                         None if slots is None else slots.data_ptr(), M, None if count is None else count.data_ptr(),
                                         _stream_ptr()))

    def erased(self):
        """(streams,) int32 view: the samples concealed so far in the running erasure; 0 where none runs."""
        return self.rec[:, 2]

    def lag(self):
        """(streams,) int32 view: the lag of the running or last erasure."""
        return self.rec[:, 1]

    def events(self):
        """(streams, 2) int32: erasures and lost packets so far (each modulo 65536).  No synchronisation."""
        import torch
        ev = self.rec[:, 3]
        return torch.stack([ev & 0xFFFF, (ev >> 16) & 0xFFFF], 1)

    def history(self):
        """(streams, Lh) int16: the histories in logical order, the newest sample last."""
        import torch
        idx = (self.rec[:, 0:1].long() + torch.arange(self.history_len, device=self.device)) % self.history_len
        return torch.gather(self.hist, 1, idx)
