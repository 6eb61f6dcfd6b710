"""Training batches from a corpus that lives in device memory (include/gtcrn_micro_hip.h, "training batches from a
resident corpus").

Counterpart of the reference's ``DNS3Dataset`` + ``DataLoader`` + ``.to(device)`` (dataloader.py:113-170): the training
set is held as int16 on the GPU (the reference's 180 000 pairs of 10 s are 115 GB, inside one MI355X's 288 GB) and
``BatchSource.draw()`` cuts -- and, with a noise corpus, mixes -- a batch where it lies, on the current stream, inside a
captured graph if the caller wants.  Nothing here falls back to the CPU; the arithmetic is csrc/batch.hip.

With a ``RirBank`` (``rirs=``, ``p_reverb=``) a drawn share of the rows is convolved with a room impulse response before
the mix -- the DNS noisy files were synthesised from reverberant speech -- in exact integer arithmetic (csrc/reverb.hip;
"reverberant speech: exact RIR convolution" in the header).  With ``target_ms=`` the same pass also
writes the row convolved with the early part of its response -- the direct path plus ``target_ms`` milliseconds -- and ``clean``
is that: a dereverberation target ("dereverberation targets: early or direct clean").  ``target=`` mixes
noise into a caller's own paired (degraded, target) speech.

With ``active_db=`` the noise is scaled to the drawn SNR of the levels over each side's active 100 ms windows -- a short clip,
pauses and a reverberant tail no longer dilute the speech level -- by exact integer window energies (gtcrn_batch_mix_active;
"active levels" in the header).

With ``p_phone=`` a drawn share of the rows of a finished batch goes through a telephone channel: band-limited to 4 kHz by an
exact integer FIR pair (16 kHz -> 8 kHz -> 16 kHz) and, per row, through linear 8 kHz PCM, mu-law or A-law G.711 in between --
what the 8 kHz and G.711 live forms hand the model (csrc/phone.hip, a post-pass over the rows any draw form has written;
"telephone-channel rows: exact 8 kHz band + G.711" in the header).  ``phone_channel`` is the same pass for
a caller's own tensors.

Out of scope: sample rates other than 16 kHz, float corpora, streaming a corpus larger than device memory from disk; for the
telephone channel: a 300 Hz high-pass or an IRS send / receive characteristic, other codecs, packet loss and jitter, a channel in
front of the mix (speech through the phone, noise added after), corpora at 8 kHz, a per-row target; for the
active levels: an active-level ``level_db`` (the level stays the mixture's plain RMS), a threshold relative to the clip, hangover
smoothing and P.56-style envelope followers, activity labels as an output; for the reverberation: targets that need a response
of their own (a shortened-decay tail), responses longer than 16384 taps, and multichannel responses.
"""
import numpy as np

from ._lib import GtcrnError, _check, _stream_ptr, lib

PLAN_DTYPE = np.dtype([("sclip", "<i4"), ("sstart", "<i4"), ("nclip", "<i4"), ("nstart", "<i4"),
                       ("snr_db", "<f4"), ("snr_amp", "<f4"), ("lvl_db", "<f4"), ("lvl_amp", "<f4")])
RECORD_DTYPE = np.dtype([("Ss", "<i8"), ("Sn", "<i8"), ("Ssn", "<i8"), ("gn", "<f4"), ("Gf", "<f4"), ("peak", "<f4"),
                         ("flags", "<i4")])
FLAG_NOISE_ZERO, FLAG_SPEECH_ZERO, FLAG_MIX_ZERO, FLAG_LIMITED = 1, 2, 4, 8
ACTIVE_RECORD_DTYPE = np.dtype([("Ss", "<i8"), ("Sn", "<i8"), ("Ssn", "<i8"), ("As", "<i8"), ("An", "<i8"), ("Ns", "<i4"),
                                ("Nn", "<i4"), ("gn", "<f4"), ("Gf", "<f4"), ("peak", "<f4"), ("flags", "<i4")])
FLAG_SPEECH_INACTIVE, FLAG_NOISE_INACTIVE = 16, 32
ACTIVE_WINDOW_MAX = 1 << 20    # samples; a window is a multiple of 8 in 8 .. this
ACTIVE_THRESHOLD_MAX = 1 << 30
REVERB_PLAN_DTYPE = np.dtype([("rir", "<i4"), ("reserved", "<i4")])
REVERB_RECORD_DTYPE = np.dtype([("rir", "<i4"), ("ntaps", "<i4"), ("saturated", "<i4"), ("reserved", "<i4")])
REVERB_SPLIT_RECORD_DTYPE = np.dtype([("rir", "<i4"), ("ntaps", "<i4"), ("saturated", "<i4"), ("split", "<i4"),
                                      ("target_saturated", "<i4"), ("reserved", "<i4", (3,))])
PHONE_PLAN_DTYPE = np.dtype([("codec", "<i4"), ("reserved", "<i4")])
PHONE_RECORD_DTYPE = np.dtype([("codec", "<i4"), ("saturated_down", "<i4"), ("saturated_up", "<i4"), ("reserved", "<i4")])
PHONE_CODECS = {"pcm": 0, "ulaw": 1, "alaw": 2}      # gtcrn_phone_item.codec; -1: a wide-band row
PHONE_TARGETS = {"narrow": 0, "wide": 1}
REVERB_MAX_TAPS = 16384        # GTCRN_REVERB_MAX_TAPS
REVERB_TAP_MAX = 32639         # GTCRN_REVERB_TAP_MAX
_U64 = (1 << 64) - 1


def _batch_lib():
    L = lib()
    if not hasattr(L, "gtcrn_batch_plan"):
        raise GtcrnError("this library has no resident-corpus batches (gtcrn_batch_*)")
    return L


def _i64(v):
    """A Python int as the int64 that carries the same 64 bits."""
    v = int(v) & _U64
    return v - (1 << 64) if v >> 63 else v


def workspace_bytes(B, L):
    n = int(_batch_lib().gtcrn_batch_workspace_bytes(int(B), int(L)))
    if n == 0:
        raise GtcrnError(lib().gtcrn_last_error().decode())
    return n


def _active_lib():
    L = _batch_lib()
    if not hasattr(L, "gtcrn_batch_mix_active"):
        raise GtcrnError("this library has no active levels (gtcrn_batch_mix_active)")
    return L


def _active_window(window):
    w = int(window)
    if w != window or w < 8 or w > ACTIVE_WINDOW_MAX or w % 8:
        raise GtcrnError(f"active_window must be a multiple of 8 samples in 8 .. {ACTIVE_WINDOW_MAX}, got {window!r}")
    return w


def active_threshold(db):
    """The integer threshold of gtcrn_batch_mix_active for a mean-square level of ``db`` dB re full scale:
    floor(2^30 * 10^(db / 10)), computed here in double (-50 dB -> 10737).  The threshold is absolute."""
    db = float(db)
    if np.isnan(db) or db > 0.0:
        raise GtcrnError("active_db is a level re full scale: at most 0 dB")
    return int(np.floor(float(ACTIVE_THRESHOLD_MAX) * 10.0 ** (db / 10.0)))


def active_workspace_bytes(B, L, window=1600):
    n = int(_active_lib().gtcrn_batch_active_workspace_bytes(int(B), int(L), int(window)))
    if n == 0:
        raise GtcrnError(lib().gtcrn_last_error().decode())
    return n


def achieved_snr_db(records):
    """-> (active, plain), float64 [B], from an ACTIVE_RECORD_DTYPE array: the SNR of the mixture over each side's active
    windows, 10 log10((As / Ns) / (gn^2 An / Nn)) -- what ``snr_db`` of the plan asks for --, and over the whole row,
    10 log10(Ss / (gn^2 Sn)).  NaN where the row has flag 1 or 2 (a side is all zero: there is no SNR)."""
    r = np.asarray(records)
    if r.dtype != ACTIVE_RECORD_DTYPE:
        raise GtcrnError("achieved_snr_db takes ACTIVE_RECORD_DTYPE records (a source with active_db=)")
    ok = (r["flags"] & (FLAG_NOISE_ZERO | FLAG_SPEECH_ZERO)) == 0
    g2 = r["gn"].astype(np.float64) ** 2
    active, plain = np.full(r.shape, np.nan), np.full(r.shape, np.nan)
    f = lambda k: r[k][ok].astype(np.float64)      # noqa: E731
    active[ok] = 10.0 * np.log10((f("As") / f("Ns")) / (g2[ok] * f("An") / f("Nn")))
    plain[ok] = 10.0 * np.log10(f("Ss") / (g2[ok] * f("Sn")))
    return active, plain


def plan_host(speech_offsets, noise_offsets, B, L, seed, step, item0=0, granule=1, snr_db=(-5.0, 20.0),
              level_db=(-35.0, -15.0), clips=None):
    """gtcrn_batch_plan_host: the plan the device would draw for (seed, step), computed on the host from host offset
    tables (int64 arrays of n + 1 entries; noise_offsets None: no noise).  Returns a PLAN_DTYPE array of B items."""
    so = np.ascontiguousarray(speech_offsets, np.int64)
    no = None if noise_offsets is None else np.ascontiguousarray(noise_offsets, np.int64)
    cl = None if clips is None else np.ascontiguousarray(clips, np.int32)
    if cl is not None and cl.size != B:
        raise GtcrnError(f"clips must hold {B} entries, got {cl.size}")
    ss = np.array([int(seed) & _U64, int(step) & _U64], np.uint64)
    plan = np.zeros(max(int(B), 0), PLAN_DTYPE)
    _check(_batch_lib().gtcrn_batch_plan_host(
        so.ctypes.data, so.size - 1, None if no is None else no.ctypes.data, 0 if no is None else no.size - 1, int(B), int(L),
        int(item0), int(granule), float(snr_db[0]), float(snr_db[1]), float(level_db[0]), float(level_db[1]),
        None if cl is None else cl.ctypes.data, ss.ctypes.data, plan.ctypes.data if plan.size else None))
    return plan


def _reverb_lib():
    L = _batch_lib()
    if not hasattr(L, "gtcrn_batch_reverb"):
        raise GtcrnError("this library has no reverberation (gtcrn_batch_reverb*)")
    return L


def reverb_plan_host(n_rir, p_reverb, B, seed, step, item0=0):
    """gtcrn_batch_reverb_plan_host: the reverb plan the device would draw for (seed, step), computed on the host.
    Returns a REVERB_PLAN_DTYPE array of B items (rir = -1: the row stays dry)."""
    ss = np.array([int(seed) & _U64, int(step) & _U64], np.uint64)
    plan = np.zeros(max(int(B), 0), REVERB_PLAN_DTYPE)
    _check(_reverb_lib().gtcrn_batch_reverb_plan_host(int(n_rir), float(p_reverb), int(B), int(item0), ss.ctypes.data,
                                                      plan.ctypes.data if plan.size else None))
    return plan


def reverb_plan_to_device(plan, device):
    """A REVERB_PLAN_DTYPE array -> the (B, 2) int32 device tensor ``BatchSource.draw(reverb_plan=...)`` takes."""
    import torch
    p = np.ascontiguousarray(plan, REVERB_PLAN_DTYPE)
    return torch.from_numpy(p.view(np.int32).reshape(p.size, 2).copy()).to(device)


def reverb_workspace_bytes(B, L):
    n = int(_reverb_lib().gtcrn_batch_reverb_workspace_bytes(int(B), int(L)))
    if n == 0:
        raise GtcrnError(lib().gtcrn_last_error().decode())
    return n


def _split_lib():
    L = _reverb_lib()
    if not hasattr(L, "gtcrn_batch_reverb_split"):
        raise GtcrnError("this library has no dereverberation targets (gtcrn_batch_reverb_split, gtcrn_batch_mix_target)")
    return L


def reverb_split_workspace_bytes(B, L):
    n = int(_split_lib().gtcrn_batch_reverb_split_workspace_bytes(int(B), int(L)))
    if n == 0:
        raise GtcrnError(lib().gtcrn_last_error().decode())
    return n


def split_for(responses, target_ms):
    """The split of each int16 response for a target of the direct path plus ``target_ms`` milliseconds:
    E_r = min(K_r, d_r + 1 + rint(16 * target_ms)), d_r the first tap of the largest magnitude (0 for a bank made with
    trim_direct=True).  target_ms = 0: the direct path alone.  -> int32 array."""
    t = float(target_ms)
    if not np.isfinite(t) or t < 0.0:
        raise GtcrnError("target_ms must be finite and not negative")
    more = int(np.rint(16.0 * t))
    out = np.zeros(len(responses), np.int32)
    for r, h in enumerate(responses):
        h = np.asarray(h)
        d = int(np.argmax(np.abs(h.astype(np.int64))))
        out[r] = min(h.size, d + 1 + more)
    return out


def plan_to_device(plan, device):
    """A PLAN_DTYPE array -> the (B, 8) int32 device tensor ``BatchSource.draw(plan=...)`` takes."""
    import torch
    p = np.ascontiguousarray(plan, PLAN_DTYPE)
    return torch.from_numpy(p.view(np.int32).reshape(p.size, 8).copy()).to(device)


def _phone_lib():
    L = _batch_lib()
    if not hasattr(L, "gtcrn_batch_phone"):
        raise GtcrnError("this library has no telephone-channel rows (gtcrn_batch_phone*)")
    return L


def _phone_mask(codecs):
    """Codec names -> gtcrn_batch_phone_plan's codec_mask."""
    names = (codecs,) if isinstance(codecs, str) else tuple(codecs)
    if not names or any(c not in PHONE_CODECS for c in names):
        raise GtcrnError(f"phone_codecs holds one or more of {tuple(PHONE_CODECS)}, got {codecs!r}")
    mask = 0
    for c in names:
        mask |= 1 << PHONE_CODECS[c]
    return mask


def _phone_target(target):
    if target not in PHONE_TARGETS:
        raise GtcrnError(f'phone_target is "narrow" or "wide", got {target!r}')
    return PHONE_TARGETS[target]


def phone_taps():
    """gtcrn_batch_phone_taps: the 129 integer taps of the channel's filter pair, exactly as the kernel uses them (int32)."""
    t = np.zeros(129, np.int32)
    if _check(_phone_lib().gtcrn_batch_phone_taps(t.ctypes.data)) != 129:
        raise GtcrnError("gtcrn_batch_phone_taps did not return 129 taps")
    return t


def phone_chunk():
    """gtcrn_batch_phone_chunk: consecutive output samples of one workgroup of the channel kernel."""
    return int(_phone_lib().gtcrn_batch_phone_chunk())


def phone_plan_host(p_phone, codecs, B, seed, step, item0=0):
    """gtcrn_batch_phone_plan_host: the phone plan the device would draw for (seed, step), computed on the host.  codecs: names
    from PHONE_CODECS, or the integer mask.  Returns a PHONE_PLAN_DTYPE array of B items (codec = -1: a wide-band row)."""
    mask = int(codecs) if isinstance(codecs, (int, np.integer)) else _phone_mask(codecs)
    ss = np.array([int(seed) & _U64, int(step) & _U64], np.uint64)
    plan = np.zeros(max(int(B), 0), PHONE_PLAN_DTYPE)
    _check(_phone_lib().gtcrn_batch_phone_plan_host(float(p_phone), mask, int(B), int(item0), ss.ctypes.data,
                                                    plan.ctypes.data if plan.size else None))
    return plan


def phone_plan_to_device(plan, device):
    """A PHONE_PLAN_DTYPE array -> the (B, 2) int32 device tensor ``BatchSource.draw(phone_plan=...)`` takes."""
    import torch
    p = np.ascontiguousarray(plan, PHONE_PLAN_DTYPE)
    return torch.from_numpy(p.view(np.int32).reshape(p.size, 2).copy()).to(device)


def phone_channel_host(noisy, clean=None, plan=None, target="narrow"):
    """gtcrn_batch_phone_host: the channel on host arrays, by the very functions the kernel compiles.  noisy, clean: (B, L)
    float32 arrays (clean may be None); plan: a PHONE_PLAN_DTYPE array of B items.  -> (noisy, clean or None, records)."""
    src_n = np.ascontiguousarray(noisy, np.float32)
    if src_n.ndim != 2:
        raise GtcrnError("noisy must be a (B, L) array")
    B, L = src_n.shape
    src_c = None if clean is None else np.ascontiguousarray(clean, np.float32)
    if src_c is not None and src_c.shape != src_n.shape:
        raise GtcrnError("clean must have noisy's shape")
    pl = np.ascontiguousarray(plan, PHONE_PLAN_DTYPE)
    if pl.shape != (B,):
        raise GtcrnError(f"plan must hold {B} items")
    out_n = np.empty_like(src_n)
    out_c = None if src_c is None else np.empty_like(src_c)
    rec = np.zeros(B, PHONE_RECORD_DTYPE)
    _check(_phone_lib().gtcrn_batch_phone_host(
        src_n.ctypes.data, L, None if src_c is None else src_c.ctypes.data, L, pl.ctypes.data, B, L, out_n.ctypes.data, L,
        None if out_c is None else out_c.ctypes.data, L, _phone_target(target), rec.ctypes.data))
    return out_n, out_c, rec


def _phone_rows(t, what, like=None):
    """(tensor, row stride) of a (B, L) float32 device tensor with contiguous rows."""
    import torch
    if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.numel() == 0
            or (t.shape[1] > 1 and t.stride(1) != 1)):
        raise GtcrnError(f"{what} must be a (B, L) float32 CUDA (ROCm) tensor with contiguous rows")
    if like is not None and (t.device != like.device or tuple(t.shape) != tuple(like.shape)):
        raise GtcrnError(f"{what} must have the noisy tensor's shape and device")
    stride = t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])
    if stride < t.shape[1]:
        raise GtcrnError(f"{what}: rows overlap")
    return t, stride


def phone_channel(noisy, clean=None, codec="ulaw", target="narrow", out=None, records=None):
    """gtcrn_batch_phone on a caller's tensors, e.g. test audio for the 8 kHz live forms: (B, L) float32 device tensors
    (clean may be None).  codec: a name from PHONE_CODECS for every row, or a (B, 2) int32 device tensor of gtcrn_phone_item
    rows (codec -1: the row is copied).  target: "narrow" (clean goes through the band, no codec) or "wide" (clean is
    copied).  out: the tensor, or the (noisy, clean) pair, to write (not the inputs: the channel is not in place); records:
    a (B, 4) int32 tensor.  -> (noisy, clean or None, records).  Asynchronous on the current stream; allocates only what
    is not given."""
    import torch
    L_ = _phone_lib()
    tg = _phone_target(target)
    (noisy, ns) = _phone_rows(noisy, "noisy")
    B, L = noisy.shape
    cs = 0
    if clean is not None:
        clean, cs = _phone_rows(clean, "clean", noisy)
    if isinstance(codec, str):
        if codec not in PHONE_CODECS:
            raise GtcrnError(f"codec is one of {tuple(PHONE_CODECS)} or a plan tensor, got {codec!r}")
        plan = torch.tensor([[PHONE_CODECS[codec], 0]], device=noisy.device, dtype=torch.int32).repeat(B, 1)
    else:
        plan = codec
        if (not isinstance(plan, torch.Tensor) or plan.device != noisy.device or plan.dtype != torch.int32
                or tuple(plan.shape) != (B, 2) or not plan.is_contiguous()):
            raise GtcrnError(f"a codec plan must be a contiguous ({B}, 2) int32 tensor on {noisy.device}")
    if out is None:
        out_n, out_c = torch.empty_like(noisy, memory_format=torch.contiguous_format), None
        if clean is not None:
            out_c = torch.empty_like(clean, memory_format=torch.contiguous_format)
    else:
        out_n, out_c = (out, None) if clean is None else out
    (out_n, ons) = _phone_rows(out_n, "out noisy", noisy)
    ocs = 0
    if clean is not None:
        out_c, ocs = _phone_rows(out_c, "out clean", noisy)
    if records is None:
        records = torch.zeros((B, 4), device=noisy.device, dtype=torch.int32)
    elif (not isinstance(records, torch.Tensor) or records.device != noisy.device or records.dtype != torch.int32
          or tuple(records.shape) != (B, 4) or not records.is_contiguous()):
        raise GtcrnError(f"records must be a contiguous ({B}, 4) int32 tensor on {noisy.device}")
    with torch.cuda.device(noisy.device):
        _check(L_.gtcrn_batch_phone(noisy.data_ptr(), ns, clean.data_ptr() if clean is not None else None, cs, plan.data_ptr(), B, L,
                                    out_n.data_ptr(), ons, out_c.data_ptr() if out_c is not None else None, ocs, tg,
                                    records.data_ptr(), _stream_ptr()))
    return out_n, out_c, records


class Corpus:
    """int16 clips back to back in one device buffer: ``pcm`` (int16, 1-D) and ``offsets`` (int64, n + 1; clip c is
    pcm[offsets[c]:offsets[c + 1]]), both caller-visible device tensors."""

    def __init__(self, pcm, offsets):
        import torch
        if not isinstance(pcm, torch.Tensor) or not pcm.is_cuda or pcm.dtype != torch.int16 or pcm.dim() != 1 or not pcm.is_contiguous():
            raise GtcrnError("pcm must be a contiguous 1-D int16 CUDA (ROCm) tensor")
        if (not isinstance(offsets, torch.Tensor) or offsets.device != pcm.device or offsets.dtype != torch.int64
                or offsets.dim() != 1 or not offsets.is_contiguous()):
            raise GtcrnError("offsets must be a contiguous 1-D int64 tensor on pcm's device")
        n = offsets.numel() - 1
        if n < 1:
            raise GtcrnError("the corpus is empty")
        if n >= 1 << 31:
            raise GtcrnError("a corpus holds fewer than 2^31 clips")
        lens = offsets[1:] - offsets[:-1]                     # checked once, here (one synchronisation)
        lo, hi = int(lens.min()), int(lens.max())
        if int(offsets[0]) < 0 or int(offsets[-1]) > pcm.numel() or lo < 1 or hi >= 1 << 31:
            raise GtcrnError("offsets must rise by 1 .. 2^31 - 1 samples per clip and stay inside pcm")
        self.pcm, self.offsets, self.n = pcm, offsets, n

    @property
    def device(self):
        return self.pcm.device

    @classmethod
    def from_tensors(cls, pcm, offsets):
        return cls(pcm, offsets)

    @classmethod
    def from_arrays(cls, arrays, device="cuda"):
        import torch
        arrays = [np.asarray(a) for a in arrays]
        for a in arrays:
            if a.dtype != np.int16 or a.ndim != 1 or a.size < 1:
                raise GtcrnError("every clip must be a 1-D int16 array of at least one sample")
        if not arrays:
            raise GtcrnError("the corpus is empty")
        off = np.zeros(len(arrays) + 1, np.int64)
        np.cumsum([a.size for a in arrays], out=off[1:])
        return cls(torch.from_numpy(np.concatenate(arrays)).to(device), torch.from_numpy(off).to(device))

    @classmethod
    def from_wavs(cls, paths, device="cuda"):
        """16 kHz mono 16-bit PCM files (the reference's data), read with the reader infer.py uses."""
        from scipy.io import wavfile
        clips = []
        for p in paths:
            fs, x = wavfile.read(p, mmap=True)
            if fs != 16000 or x.ndim != 1 or x.dtype != np.int16:
                raise GtcrnError(f"{p}: a corpus takes 16 kHz mono 16-bit PCM, got {fs} Hz, shape {tuple(x.shape)}, {x.dtype}")
            clips.append(np.asarray(x))
        return cls.from_arrays(clips, device)

    def save(self, prefix):
        """Writes ``prefix + '.pcm.npy'`` and ``prefix + '.offsets.npy'``."""
        np.save(prefix + ".pcm.npy", self.pcm.cpu().numpy())
        np.save(prefix + ".offsets.npy", self.offsets.cpu().numpy())

    @classmethod
    def load(cls, prefix, device="cuda"):
        import torch
        pcm, off = np.load(prefix + ".pcm.npy"), np.load(prefix + ".offsets.npy")
        if pcm.dtype != np.int16 or off.dtype != np.int64 or pcm.ndim != 1 or off.ndim != 1:
            raise GtcrnError(f"{prefix}: not a saved corpus (int16 pcm, int64 offsets)")
        return cls(torch.from_numpy(pcm).to(device), torch.from_numpy(off).to(device))


def quantize_rirs(arrays, normalize="peak", trim_direct=True):
    """The host side of ``RirBank.from_arrays``: a list of 1-D responses -> a list of int16 Q15 arrays inside
    +-REVERB_TAP_MAX.  An int16 array is Q15 already and is only trimmed and checked.  A float array is scaled first:
    normalize="peak": its largest |tap| becomes REVERB_TAP_MAX / 32768 (0.996: a direct path of all but unit gain);
    normalize="energy": its taps' sum of squares becomes 1, or as near to it as the peak bound allows; then
    tap = rint(32768 * h), round half to even.  trim_direct: the taps before the direct path -- the first tap of the
    largest magnitude -- are dropped, so that a wet row is not delayed against its noise by the measurement's lead-in."""
    if normalize not in ("peak", "energy"):
        raise GtcrnError('normalize is "peak" or "energy"')
    out = []
    for k, a in enumerate(arrays):
        a = np.asarray(a)
        if a.ndim != 1 or a.size < 1:
            raise GtcrnError(f"response {k}: a 1-D array of at least one tap")
        if a.dtype == np.int16:
            q = a.astype(np.int64)
        elif a.dtype.kind == "f":
            h = a.astype(np.float64)
            if not np.isfinite(h).all():
                raise GtcrnError(f"response {k}: not finite")
            peak = np.abs(h).max()
            if peak == 0.0:
                raise GtcrnError(f"response {k}: all taps are zero")
            top = REVERB_TAP_MAX / 32768.0
            g = top / peak
            if normalize == "energy":
                g = min(g, 1.0 / np.sqrt((h * h).sum()))
            q = np.clip(np.rint(h * g * 32768.0), -REVERB_TAP_MAX, REVERB_TAP_MAX).astype(np.int64)
        else:
            raise GtcrnError(f"response {k}: float or int16 taps, got {a.dtype}")
        if trim_direct:
            q = q[int(np.argmax(np.abs(q))):]
        if q.size > REVERB_MAX_TAPS:
            raise GtcrnError(f"response {k}: {q.size} taps; at most {REVERB_MAX_TAPS} (1.024 s)")
        if np.abs(q).max() > REVERB_TAP_MAX:
            raise GtcrnError(f"response {k}: an int16 tap outside +-{REVERB_TAP_MAX}")
        out.append(q.astype(np.int16))
    if not out:
        raise GtcrnError("the bank is empty")
    return out


class RirBank:
    """Room impulse responses in device memory, shaped like a corpus: ``taps`` (int16 Q15, 1-D, the responses back to
    back) and ``offsets`` (int64, n + 1), plus ``table``, the derived tap table of the convolution's matrix form
    (gtcrn_batch_reverb_prepare, filled here, once).  Every response holds 1 .. 16384 taps inside +-32639; checked here,
    once (one synchronisation)."""

    def __init__(self, taps, offsets):
        import torch
        L = _reverb_lib()
        if not isinstance(taps, torch.Tensor) or not taps.is_cuda or taps.dtype != torch.int16 or taps.dim() != 1 or not taps.is_contiguous():
            raise GtcrnError("taps must be a contiguous 1-D int16 CUDA (ROCm) tensor")
        if (not isinstance(offsets, torch.Tensor) or offsets.device != taps.device or offsets.dtype != torch.int64
                or offsets.dim() != 1 or not offsets.is_contiguous()):
            raise GtcrnError("offsets must be a contiguous 1-D int64 tensor on taps' device")
        n = offsets.numel() - 1
        if n < 1:
            raise GtcrnError("the bank is empty")
        if n >= 1 << 31:
            raise GtcrnError("a bank holds fewer than 2^31 responses")
        off = offsets.cpu().numpy()
        lens = off[1:] - off[:-1]
        if int(off[0]) < 0 or int(off[-1]) > taps.numel() or int(lens.min()) < 1 or int(lens.max()) > REVERB_MAX_TAPS:
            raise GtcrnError(f"offsets must rise by 1 .. {REVERB_MAX_TAPS} taps per response and stay inside taps")
        used = taps[int(off[0]):int(off[-1])]
        if int(used.min()) < -REVERB_TAP_MAX or int(used.max()) > REVERB_TAP_MAX:
            raise GtcrnError(f"every tap must lie in +-{REVERB_TAP_MAX}")
        self.taps, self.offsets, self.n = taps, offsets, n
        self._host_offsets, self._split_tables = off.astype(np.int64), {}
        nbytes = int(L.gtcrn_batch_reverb_table_bytes(off.ctypes.data, n))
        if nbytes == 0:
            raise GtcrnError(lib().gtcrn_last_error().decode())
        self.table = torch.empty(nbytes, device=taps.device, dtype=torch.uint8)
        with torch.cuda.device(taps.device):
            _check(L.gtcrn_batch_reverb_prepare(taps.data_ptr(), offsets.data_ptr(), n, self.table.data_ptr(), nbytes, _stream_ptr()))

    @property
    def device(self):
        return self.taps.device

    def split_for(self, target_ms):
        """int32 [n]: per response the number of leading taps that make a target of the direct path plus ``target_ms``
        milliseconds (``data.split_for`` on this bank's taps; reads them back once per call)."""
        taps, off = self.taps.cpu().numpy(), self._host_offsets
        return split_for([taps[int(off[r]):int(off[r + 1])] for r in range(self.n)], target_ms)

    def split_table(self, split):
        """-> (split, table): the int32 device split and the split table of gtcrn_batch_reverb_split_prepare for it, made
        once per split and kept.  A value outside 1 .. K_r is clamped into it, as the library does."""
        import torch
        L = _split_lib()
        sp = np.ascontiguousarray(split, np.int32)
        if sp.ndim != 1 or sp.size != self.n:
            raise GtcrnError(f"split must hold {self.n} entries")
        lens = (self._host_offsets[1:] - self._host_offsets[:-1]).astype(np.int64)
        sp = np.clip(sp, 1, lens).astype(np.int32)
        key = sp.tobytes()
        if key not in self._split_tables:
            nbytes = int(L.gtcrn_batch_reverb_split_table_bytes(self._host_offsets.ctypes.data, sp.ctypes.data, self.n))
            if nbytes == 0:
                raise GtcrnError(lib().gtcrn_last_error().decode())
            d_split = torch.from_numpy(sp).to(self.device)
            table = torch.empty(nbytes, device=self.device, dtype=torch.uint8)
            with torch.cuda.device(self.device):
                _check(L.gtcrn_batch_reverb_split_prepare(self.taps.data_ptr(), self.offsets.data_ptr(), d_split.data_ptr(), self.n,
                                                          table.data_ptr(), nbytes, _stream_ptr()))
            self._split_tables[key] = (d_split, table)
        return self._split_tables[key]

    @classmethod
    def from_tensors(cls, taps, offsets):
        return cls(taps, offsets)

    @classmethod
    def from_arrays(cls, arrays, normalize="peak", trim_direct=True, device="cuda"):
        import torch
        q = quantize_rirs(arrays, normalize, trim_direct)
        off = np.zeros(len(q) + 1, np.int64)
        np.cumsum([a.size for a in q], out=off[1:])
        return cls(torch.from_numpy(np.concatenate(q)).to(device), torch.from_numpy(off).to(device))

    @classmethod
    def from_wavs(cls, paths, normalize="peak", trim_direct=True, device="cuda"):
        """16 kHz mono files, 16-bit PCM or float, each one response."""
        from scipy.io import wavfile
        hs = []
        for p in paths:
            fs, x = wavfile.read(p, mmap=True)
            if fs != 16000 or x.ndim != 1:
                raise GtcrnError(f"{p}: a bank takes 16 kHz mono files, got {fs} Hz, shape {tuple(x.shape)}")
            hs.append(np.asarray(x, np.float64) / 32768.0 if x.dtype == np.int16 else np.asarray(x))
        return cls.from_arrays(hs, normalize, trim_direct, device)

    def save(self, prefix):
        """Writes ``prefix + '.taps.npy'`` and ``prefix + '.offsets.npy'`` (the table is derived again on load)."""
        np.save(prefix + ".taps.npy", self.taps.cpu().numpy())
        np.save(prefix + ".offsets.npy", self.offsets.cpu().numpy())

    @classmethod
    def load(cls, prefix, device="cuda"):
        import torch
        taps, off = np.load(prefix + ".taps.npy"), np.load(prefix + ".offsets.npy")
        if taps.dtype != np.int16 or off.dtype != np.int64 or taps.ndim != 1 or off.ndim != 1:
            raise GtcrnError(f"{prefix}: not a saved bank (int16 taps, int64 offsets)")
        return cls(torch.from_numpy(taps).to(device), torch.from_numpy(off).to(device))


class BatchSource:
    """Draws (noisy, clean) batches of B rows of L samples from resident corpora.

    ``noise=`` a second Corpus: dynamic mixing of ``speech`` with wrapped noise at an SNR from U(snr_db) and a mixture
    level from U(level_db) dB RMS re full scale (gtcrn_batch_mix).  ``paired_clean=`` a Corpus under the same offsets
    table as ``speech`` (which is then the noisy side): the reference's loader, exactly (gtcrn_batch_pairs).
    A batch is a pure function of (seed, step, item0 + row); ``item0`` = rank * B makes ranks cut one global batch.
    granule = 1: sample-exact starts; 16000: the reference's whole-second random_start.
    ``rirs=`` a RirBank (mix form only): each row is reverberant with probability ``p_reverb`` -- its speech window, with
    its true history, convolved with a drawn response (gtcrn_batch_reverb) -- and ``clean`` is then the reverberant
    speech.  With p_reverb = 0 every draw is bit-identical to the source without ``rirs=``.  ``reverb_form``: gtcrn_batch_reverb's
    `form` (0: the library chooses; 1 plain, 2 matrix, 3 / 4 matrix with the block pinned: bit-identical, for measurements).
    ``target_ms=`` a number (with ``rirs=``): ``clean`` is the speech convolved with the early part of the row's response, the
    direct path plus ``target_ms`` milliseconds (0: the direct path alone; ``RirBank.split_for``), written by the same pass as
    the wet row (gtcrn_batch_reverb_split, gtcrn_batch_mix_target); ``noisy``, its SNR and its level are those of the fully
    reverberant speech.  None: the draw above, call for call.
    ``target=`` a Corpus under ``speech``'s offsets table (mix form, without ``rirs=``): ``clean`` is cut from it instead of
    from ``speech`` -- noise mixed on the device into a caller's own paired (degraded, target) speech.
    ``active_db=`` a level in dB re full scale (mix form; -50 is the usual choice): the drawn SNR is that of the levels over the
    windows of ``active_window`` samples (1600: 100 ms) whose mean square exceeds it, each side by its own activity
    (gtcrn_batch_mix_active in place of the two mix calls above, in every combination with ``rirs=``, ``target_ms=`` and
    ``target=``).  ``records`` is then (B, 16) int32, ``records_numpy()`` ACTIVE_RECORD_DTYPE, ``active_threshold`` the integer
    threshold; ``achieved_snr_db`` reads the SNR back.  None: the draw above, call for call.
    ``p_phone=`` (every form above): each row of the finished batch is a telephone row with that probability -- band-limited to
    4 kHz and passed through one of ``phone_codecs`` ("pcm": linear 8 kHz PCM, "ulaw", "alaw"), drawn per row (gtcrn_batch_phone,
    a post-pass: the draw above runs unchanged into two raw buffers the source owns, the channel writes ``noisy`` / ``clean``).
    ``phone_target``: "narrow" -- ``clean`` of a telephone row is band-limited too, without the codec -- or "wide" -- it stays
    as drawn.  ``phone_plan`` is the drawn (B, 2) int32 plan, ``phone_records_numpy()`` the records.  0: the draw above, call for
    call, and nothing more is allocated."""

    def __init__(self, speech, noise=None, paired_clean=None, B=1, L=64000, seed=0, snr_db=(-5.0, 20.0), level_db=(-35.0, -15.0),
                 granule=1, item0=0, rirs=None, p_reverb=0.0, reverb_form=0, target_ms=None, target=None, active_db=None,
                 active_window=1600, p_phone=0.0, phone_codecs=("pcm", "ulaw", "alaw"), phone_target="narrow"):
        import torch
        _batch_lib()
        self.p_phone, self.phone_mask, self.phone_target = float(p_phone), _phone_mask(phone_codecs), phone_target
        _phone_target(phone_target)
        if not 0.0 <= self.p_phone <= 1.0:               # (a NaN fails both comparisons)
            raise GtcrnError("p_phone must lie in 0 .. 1")
        if self.p_phone > 0.0:
            _phone_lib()
        if (noise is None) == (paired_clean is None):
            raise GtcrnError("give exactly one of noise= (mix) and paired_clean= (pairs)")
        self.active_db, self.active_window, self.active_threshold = None, None, None
        if active_db is not None:                        # decided on the arguments alone, before any corpus is looked at
            _active_lib()
            if paired_clean is not None:
                raise GtcrnError("active_db= goes with noise= (the mix): a paired corpus is not mixed, so it has no SNR to set")
            self.active_window = _active_window(active_window)
            self.active_db, self.active_threshold = float(active_db), active_threshold(active_db)
        other = noise if noise is not None else paired_clean
        if not isinstance(speech, Corpus) or not isinstance(other, Corpus) or other.device != speech.device:
            raise GtcrnError("the corpora must be data.Corpus objects on one device")
        if paired_clean is not None and (paired_clean.n != speech.n or not torch.equal(paired_clean.offsets, speech.offsets)):
            raise GtcrnError("paired corpora must share one offsets table")
        B, L, granule, item0 = int(B), int(L), int(granule), int(item0)
        self.snr_db = (float(snr_db[0]), float(snr_db[1]))
        self.level_db = (float(level_db[0]), float(level_db[1]))
        if B < 1 or L < 1 or L >= 1 << 31:
            raise GtcrnError("B and L must be positive (L below 2^31)")
        if granule < 1:
            raise GtcrnError("granule must be at least 1")
        if self.snr_db[1] < self.snr_db[0] or self.level_db[1] < self.level_db[0]:
            raise GtcrnError("a range has hi < lo")
        if item0 < 0 or item0 + B > 1 << 32:
            raise GtcrnError("item0 .. item0 + B must lie in 0 .. 2^32")
        self.speech, self.noise, self.paired_clean = speech, noise, paired_clean
        self.B, self.L, self.granule, self.item0 = B, L, granule, item0
        dev = self.device = speech.device
        self.plan = torch.zeros((B, 8), device=dev, dtype=torch.int32)          # gtcrn_batch_item rows
        self.records = torch.zeros((B, 10), device=dev, dtype=torch.int32)      # gtcrn_batch_record rows (mix only)
        self.seed_step = torch.tensor([_i64(seed), 0], device=dev, dtype=torch.int64)
        self.noisy = torch.empty((B, L), device=dev, dtype=torch.float32)
        self.clean = torch.empty((B, L), device=dev, dtype=torch.float32)
        self._ws = torch.empty(workspace_bytes(B, L), device=dev, dtype=torch.uint8) if noise is not None else None
        if self.active_db is not None:
            self.records = torch.zeros((B, 16), device=dev, dtype=torch.int32)  # gtcrn_batch_active_record rows
            self._ws = torch.empty(active_workspace_bytes(B, L, self.active_window), device=dev, dtype=torch.uint8)
        self.rirs, self.p_reverb, self.reverb_form = rirs, float(p_reverb), int(reverb_form)
        self.target, self.target_ms = target, None if target_ms is None else float(target_ms)
        if target is not None:
            _split_lib()
            if noise is None or rirs is not None:
                raise GtcrnError("target= goes with noise= (the mix) and without rirs= or paired_clean=")
            if not isinstance(target, Corpus) or target.device != speech.device:
                raise GtcrnError("target must be a data.Corpus on the corpora's device")
            if target.n != speech.n or not torch.equal(target.offsets, speech.offsets):
                raise GtcrnError("target and speech must share one offsets table")
        if target_ms is not None and rirs is None:
            raise GtcrnError("target_ms needs rirs=")
        if rirs is not None:
            _reverb_lib()
            if paired_clean is not None:
                raise GtcrnError("rirs= goes with noise= (the mix); a paired corpus is what it is")
            if not isinstance(rirs, RirBank) or rirs.device != dev:
                raise GtcrnError("rirs must be a data.RirBank on the corpora's device")
            if not 0.0 <= self.p_reverb <= 1.0:
                raise GtcrnError("p_reverb must lie in 0 .. 1")
            if self.reverb_form not in (0, 1, 2, 3, 4):
                raise GtcrnError("reverb_form is 0 (the library chooses), 1 (plain), 2 (matrix) or 3 / 4 (matrix, block pinned)")
            self.staged_stride = (L + 7) // 8 * 8                                # rows of whole 16 bytes
            self.staged = torch.zeros(B * self.staged_stride, device=dev, dtype=torch.int16)
            self.staged_offsets = torch.zeros(B + 1, device=dev, dtype=torch.int64)
            self.staged_plan = torch.zeros((B, 8), device=dev, dtype=torch.int32)
            self.reverb_plan = torch.full((B, 2), -1, device=dev, dtype=torch.int32)   # gtcrn_reverb_item rows
            self.reverb_records = torch.zeros((B, 4), device=dev, dtype=torch.int32)   # gtcrn_reverb_record rows
            self._rws = torch.empty(reverb_workspace_bytes(B, L), device=dev, dtype=torch.uint8)
            if target_ms is not None:
                _split_lib()
                self.split, self.split_table = rirs.split_table(rirs.split_for(self.target_ms))
                self.staged_target = torch.zeros(B * self.staged_stride, device=dev, dtype=torch.int16)
                self.split_records = torch.zeros((B, 8), device=dev, dtype=torch.int32)   # gtcrn_reverb_split_record rows
                self._rws = torch.empty(reverb_split_workspace_bytes(B, L), device=dev, dtype=torch.uint8)
        elif self.p_reverb != 0.0:
            raise GtcrnError("p_reverb needs rirs=")
        self.phone_plan = self.phone_records = None
        if self.p_phone > 0.0:
            ls = (L + 3) // 4 * 4                        # raw rows of whole 16 bytes
            self._raw_noisy = torch.empty((B, ls), device=dev, dtype=torch.float32)[:, :L]
            self._raw_clean = torch.empty((B, ls), device=dev, dtype=torch.float32)[:, :L]
            self.phone_plan = torch.full((B, 2), -1, device=dev, dtype=torch.int32)    # gtcrn_phone_item rows
            self.phone_records = torch.zeros((B, 4), device=dev, dtype=torch.int32)    # gtcrn_phone_record rows

    # ---- the step word ----------------------------------------------------------------------------------------------
    def set_step(self, k):
        """The next drawn plan is step k's (stream-ordered, for a resume)."""
        self.seed_step[1:2].fill_(_i64(k))

    def step(self):
        """The step the next drawn plan will use (reads the device word: synchronises)."""
        return int(self.seed_step[1].item()) & _U64

    def plan_numpy(self):
        return self.plan.cpu().numpy().view(PLAN_DTYPE).reshape(self.B)

    def records_numpy(self):
        """The mix records of the most recent draw: RECORD_DTYPE, or ACTIVE_RECORD_DTYPE for a source with ``active_db=``."""
        return self.records.cpu().numpy().view(RECORD_DTYPE if self.active_db is None else ACTIVE_RECORD_DTYPE).reshape(self.B)

    def reverb_plan_numpy(self):
        """The reverb plan of the most recent draw (a source with ``rirs=``)."""
        return self.reverb_plan.cpu().numpy().view(REVERB_PLAN_DTYPE).reshape(self.B)

    def reverb_records_numpy(self):
        if self.target_ms is not None:                   # the split records' first three fields are these records'
            s, out = self.split_records_numpy(), np.zeros(self.B, REVERB_RECORD_DTYPE)
            for f in ("rir", "ntaps", "saturated"):
                out[f] = s[f]
            return out
        return self.reverb_records.cpu().numpy().view(REVERB_RECORD_DTYPE).reshape(self.B)

    def split_records_numpy(self):
        """The split records of the most recent draw (a source with ``target_ms=``)."""
        return self.split_records.cpu().numpy().view(REVERB_SPLIT_RECORD_DTYPE).reshape(self.B)

    def phone_plan_numpy(self):
        """The phone plan of the most recent draw (a source with ``p_phone`` > 0)."""
        if self.phone_plan is None:
            raise GtcrnError("phone_plan_numpy needs a source with p_phone > 0")
        return self.phone_plan.cpu().numpy().view(PHONE_PLAN_DTYPE).reshape(self.B)

    def phone_records_numpy(self):
        """The phone records of the most recent draw (a source with ``p_phone`` > 0)."""
        if self.phone_records is None:
            raise GtcrnError("phone_records_numpy needs a source with p_phone > 0")
        return self.phone_records.cpu().numpy().view(PHONE_RECORD_DTYPE).reshape(self.B)

    # ---- drawing ----------------------------------------------------------------------------------------------------
    def _rows(self, t, what):
        import torch
        if (not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != torch.float32 or t.dim() != 2
                or tuple(t.shape) != (self.B, self.L) or (self.L > 1 and t.stride(1) != 1)):
            raise GtcrnError(f"{what} must be a ({self.B}, {self.L}) float32 tensor on {self.device} with contiguous rows")
        stride = t.stride(0) if self.B > 1 else max(t.stride(0), self.L)      # (a one-row tensor may report any stride)
        if stride < self.L:
            raise GtcrnError(f"{what}: rows overlap (stride {stride} < {self.L})")
        return t, stride

    def draw_plan(self, clips=None, advance=True):
        """Fills ``self.plan`` for the current (seed, step) and, with advance, moves the step word on by one.  clips: an
        int32 device tensor of B clip ids (e.g. a slice of ``torch.randperm(n, device=...)``: an epoch without
        replacement) instead of drawn ones."""
        import torch
        if clips is not None and (not isinstance(clips, torch.Tensor) or clips.device != self.device or clips.dtype != torch.int32
                                  or clips.dim() != 1 or clips.numel() != self.B or not clips.is_contiguous()):
            raise GtcrnError(f"clips must be a contiguous int32 tensor of {self.B} ids on {self.device}")
        nz = self.noise
        with torch.cuda.device(self.device):
            _check(lib().gtcrn_batch_plan(
                self.speech.offsets.data_ptr(), self.speech.n, nz.offsets.data_ptr() if nz is not None else None,
                nz.n if nz is not None else 0, self.B, self.L, self.item0, self.granule, self.snr_db[0], self.snr_db[1],
                self.level_db[0], self.level_db[1], clips.data_ptr() if clips is not None else None,
                self.seed_step.data_ptr(), int(bool(advance)), self.plan.data_ptr(), _stream_ptr()))
        return self.plan

    def draw_reverb_plan(self):
        """Fills ``self.reverb_plan`` for the current (seed, step); the step word is read, never moved (so this goes
        before ``draw_plan``)."""
        import torch
        with torch.cuda.device(self.device):
            _check(lib().gtcrn_batch_reverb_plan(self.rirs.n, self.p_reverb, self.B, self.item0, self.seed_step.data_ptr(),
                                                 self.reverb_plan.data_ptr(), _stream_ptr()))
        return self.reverb_plan

    def draw_phone_plan(self):
        """Fills ``self.phone_plan`` for the current (seed, step); the step word is read, never moved (so this goes before
        ``draw_plan``)."""
        import torch
        if self.phone_plan is None:
            raise GtcrnError("draw_phone_plan needs a source with p_phone > 0")
        with torch.cuda.device(self.device):
            _check(lib().gtcrn_batch_phone_plan(self.p_phone, self.phone_mask, self.B, self.item0, self.seed_step.data_ptr(),
                                                self.phone_plan.data_ptr(), _stream_ptr()))
        return self.phone_plan

    def draw(self, clips=None, plan=None, out=None, passes=7, reverb_plan=None, phone_plan=None):
        """-> (noisy, clean), (B, L) float32: ``self.noisy`` / ``self.clean`` or the pair given as ``out`` (row strides
        >= L).  plan: a (B, 8) int32 device tensor of gtcrn_batch_item rows to use instead of drawing one (the step word
        then stays).  reverb_plan (a source with ``rirs=``): a (B, 2) int32 device tensor of gtcrn_reverb_item rows to use
        instead of drawing one.  phone_plan (a source with ``p_phone`` > 0): a (B, 2) int32 device tensor of gtcrn_phone_item
        rows to use instead of drawing one.  Asynchronous on the current stream, allocates nothing, capturable.  passes:
        measurement hook of the mix form (gtcrn_batch_mix)."""
        import torch
        if self.phone_plan is None:
            if phone_plan is not None:
                raise GtcrnError("phone_plan= needs a source with p_phone > 0")
            return self._draw_rows(clips, plan, out, passes, reverb_plan)
        if phone_plan is None:
            pp = self.draw_phone_plan()                  # before the batch plan: that one moves the step word
        else:
            pp = phone_plan
            if (not isinstance(pp, torch.Tensor) or pp.device != self.device or pp.dtype != torch.int32
                    or tuple(pp.shape) != (self.B, 2) or not pp.is_contiguous()):
                raise GtcrnError(f"phone_plan must be a contiguous ({self.B}, 2) int32 tensor on {self.device}")
        noisy, clean = (self.noisy, self.clean) if out is None else out
        (noisy, ns), (clean, cs) = self._rows(noisy, "noisy"), self._rows(clean, "clean")
        raw_n, raw_c = self._draw_rows(clips, plan, (self._raw_noisy, self._raw_clean), passes, reverb_plan)
        with torch.cuda.device(self.device):
            _check(lib().gtcrn_batch_phone(raw_n.data_ptr(), raw_n.stride(0), raw_c.data_ptr(), raw_c.stride(0), pp.data_ptr(),
                                           self.B, self.L, noisy.data_ptr(), ns, clean.data_ptr(), cs,
                                           PHONE_TARGETS[self.phone_target], self.phone_records.data_ptr(), _stream_ptr()))
        return noisy, clean

    def _draw_rows(self, clips, plan, out, passes, reverb_plan):
        """The draw without the telephone channel: every form of the class docstring, into ``out``."""
        import torch
        rp = None
        if reverb_plan is not None:
            if self.rirs is None:
                raise GtcrnError("reverb_plan= needs a source with rirs=")
            rp = reverb_plan
            if (not isinstance(rp, torch.Tensor) or rp.device != self.device or rp.dtype != torch.int32
                    or tuple(rp.shape) != (self.B, 2) or not rp.is_contiguous()):
                raise GtcrnError(f"reverb_plan must be a contiguous ({self.B}, 2) int32 tensor on {self.device}")
        elif self.rirs is not None:
            rp = self.draw_reverb_plan()                 # before the batch plan: that one moves the step word
        if plan is None:
            p = self.draw_plan(clips)
        else:
            if clips is not None:
                raise GtcrnError("give clips= or plan=, not both")
            p = plan
            if (not isinstance(p, torch.Tensor) or p.device != self.device or p.dtype != torch.int32
                    or tuple(p.shape) != (self.B, 8) or not p.is_contiguous()):
                raise GtcrnError(f"plan must be a contiguous ({self.B}, 8) int32 tensor on {self.device}")
        noisy, clean = (self.noisy, self.clean) if out is None else out
        (noisy, ns), (clean, cs) = self._rows(noisy, "noisy"), self._rows(clean, "clean")
        sp = self.speech
        with torch.cuda.device(self.device):
            if self.noise is not None:
                nz = self.noise
                s_pcm, s_off, s_n = sp.pcm, sp.offsets, sp.n
                t_pcm = self.target.pcm if self.target is not None else None
                if rp is not None and self.target_ms is not None:      # one pass, two staged corpora: wet speech and its target
                    rb = self.rirs
                    _check(lib().gtcrn_batch_reverb_split(
                        sp.pcm.data_ptr(), sp.offsets.data_ptr(), sp.n, rb.taps.data_ptr(), rb.offsets.data_ptr(),
                        self.split.data_ptr(), rb.n, self.split_table.data_ptr(), self.split_table.numel(), p.data_ptr(),
                        rp.data_ptr(), self.B, self.L, self.staged.data_ptr(), self.staged_target.data_ptr(), self.staged_stride,
                        self.staged_offsets.data_ptr(), self.staged_plan.data_ptr(), self.split_records.data_ptr(),
                        self._rws.data_ptr(), self.reverb_form, _stream_ptr()))
                    s_pcm, s_off, s_n, p, t_pcm = self.staged, self.staged_offsets, self.B, self.staged_plan, self.staged_target
                elif rp is not None:                     # the speech side of the mix becomes the staged corpus
                    rb = self.rirs
                    _check(lib().gtcrn_batch_reverb(
                        sp.pcm.data_ptr(), sp.offsets.data_ptr(), sp.n, rb.taps.data_ptr(), rb.offsets.data_ptr(), rb.n,
                        rb.table.data_ptr(), rb.table.numel(), p.data_ptr(), rp.data_ptr(), self.B, self.L,
                        self.staged.data_ptr(), self.staged_stride, self.staged_offsets.data_ptr(), self.staged_plan.data_ptr(),
                        self.reverb_records.data_ptr(), self._rws.data_ptr(), self.reverb_form, _stream_ptr()))
                    s_pcm, s_off, s_n, p = self.staged, self.staged_offsets, self.B, self.staged_plan
                if self.active_db is not None:           # one entry point for the plain and the target form
                    _check(lib().gtcrn_batch_mix_active(s_pcm.data_ptr(), s_off.data_ptr(), s_n, nz.pcm.data_ptr(),
                                                        nz.offsets.data_ptr(), nz.n, t_pcm.data_ptr() if t_pcm is not None else None,
                                                        p.data_ptr(), self.B, self.L, noisy.data_ptr(), ns, clean.data_ptr(), cs,
                                                        self.active_window, self.active_threshold, self.records.data_ptr(),
                                                        self._ws.data_ptr(), int(passes), _stream_ptr()))
                elif t_pcm is not None:
                    _check(lib().gtcrn_batch_mix_target(s_pcm.data_ptr(), s_off.data_ptr(), s_n, nz.pcm.data_ptr(),
                                                        nz.offsets.data_ptr(), nz.n, t_pcm.data_ptr(), p.data_ptr(), self.B, self.L,
                                                        noisy.data_ptr(), ns, clean.data_ptr(), cs, self.records.data_ptr(),
                                                        self._ws.data_ptr(), int(passes), _stream_ptr()))
                else:
                    _check(lib().gtcrn_batch_mix(s_pcm.data_ptr(), s_off.data_ptr(), s_n, nz.pcm.data_ptr(), nz.offsets.data_ptr(),
                                                 nz.n, p.data_ptr(), self.B, self.L, noisy.data_ptr(), ns, clean.data_ptr(), cs,
                                                 self.records.data_ptr(), self._ws.data_ptr(), int(passes), _stream_ptr()))
            else:
                _check(lib().gtcrn_batch_pairs(sp.pcm.data_ptr(), self.paired_clean.pcm.data_ptr(), sp.offsets.data_ptr(), sp.n,
                                               p.data_ptr(), self.B, self.L, noisy.data_ptr(), ns, clean.data_ptr(), cs,
                                               _stream_ptr()))
        return noisy, clean
