"""Checker of the tone guard (include/gtcrn_micro_hip.h, "tone guard"): steps 1 .. 7 of the contract in numpy float32, every
operation one rounding, the reductions in the stated order.  It reproduces a device output and a device record bit for bit
from the blocks the calls WITHOUT tones emit: w (wet) and x (the dry samples under them).

`block` is steps 1 and 3 .. 5 on one record (what gtcrn_tone_block_host does) and returns the names of the branches it took
(the trace); `stream` runs the blocks of one stream through steps 1 .. 7: the structural zero of step 2, the guarded mix
with gains and ramp words, level control (tests/alc_checker.py) and the meters' sums.  `wrong=` distorts one definition at
a time: the seeded bugs the comparison must reject."""
import math

import numpy as np

import alc_checker as AK
import ramp_checker as RK

F32 = np.float32
FMAX = F32(np.finfo(np.float32).max)
FREQS = (697, 770, 852, 941, 1209, 1336, 1477, 1633, 1100, 2100)
NAMES = ("theta", "tau", "delta", "pi2", "pi1", "G", "N2", "N1", "H", "mode", "singles")
DEFAULTS = dict(min_dbov=-45.0, twist_db=8.0, dominance_db=8.0, pair_purity=0.6, single_purity=0.8, guard_blocks=1,
                digit_blocks=2, single_blocks=4, hold_blocks=1, mode=1, singles=1)
WRONG = ("purity_on_P", "pairwise", "hold_on_candidate", "twist_one_sided", "last_argmax", "events_every_block")
DIGITS = "123A456B789C*0#D"                                   # code 1 + 4 row + col -> the key


def table():
    """(10, 256, 2) float32: cos and sin of 2 pi F i / 16000, computed in double and rounded once."""
    t = np.empty((10, 256, 2), np.float32)
    for f, F in enumerate(FREQS):
        for i in range(256):
            a = 2 * math.pi * F * i / 16000
            t[f, i] = (math.cos(a), math.sin(a))
    return t


def params(**fields):
    """The 16 parameter words: double arithmetic, one rounding per word."""
    c = dict(DEFAULTS, **fields)
    p = np.zeros(16, np.float32)
    p[:11] = [256.0 * 10.0 ** (c["min_dbov"] / 10), 10.0 ** (c["twist_db"] / 10), 10.0 ** (-c["dominance_db"] / 10),
              c["pair_purity"], c["single_purity"], c["guard_blocks"], c["digit_blocks"], c["single_blocks"], c["hold_blocks"],
              c["mode"], c["singles"]]
    return p


def lane_sum(prod, pairwise=False):
    """((p0 + p1) + p2) + p3 per lane (samples 2l, 2l+1, 128+2l, 129+2l), then the xor butterfly over 1 .. 32; over the last
    axis of prod (..., 256)."""
    if pairwise:                                              # the seeded bug: numpy's own pairwise sum
        return np.sum(prod, axis=-1, dtype=np.float32)
    lane = np.arange(64)
    p = (prod[..., 2 * lane] + prod[..., 2 * lane + 1]).astype(np.float32)
    p = (p + prod[..., 128 + 2 * lane]).astype(np.float32)
    p = (p + prod[..., 129 + 2 * lane]).astype(np.float32)
    for d in (1, 2, 4, 8, 16, 32):
        p = (p + p[..., lane ^ d]).astype(np.float32)
    return p[..., 0]


def powers(x, tab, pairwise=False):
    """Step 1: E_x (...,) and P_0 .. P_9 (..., 10) of the blocks x (..., 256)."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        Ex = lane_sum((x * x).astype(np.float32), pairwise)
        c = lane_sum((x[..., None, :] * tab[:, :, 0]).astype(np.float32), pairwise)
        s = lane_sum((x[..., None, :] * tab[:, :, 1]).astype(np.float32), pairwise)
        P = ((c * c).astype(np.float32) + (s * s).astype(np.float32)).astype(np.float32)
    return Ex, P


def candidate(p, Ex, P, tr, wrong=None):
    """Step 3 -> the candidate code."""
    if not (Ex <= FMAX and all(v <= FMAX for v in P)):
        tr.add("nonfinite")
        return 0
    e = (P * F32(0.0078125)).astype(np.float32)
    rows, cols = P[:4], P[4:8]
    if wrong == "last_argmax":
        r, c = 3 - int(np.argmax(rows[::-1])), 3 - int(np.argmax(cols[::-1]))
    else:
        r, c = int(np.argmax(rows)), int(np.argmax(cols))     # (numpy's argmax is the first one)
    if (rows == rows[r]).sum() > 1 or (cols == cols[c]).sum() > 1:
        tr.add("argmax_tie")
    er, ec = e[r], e[4 + c]
    fails = []
    if not (er >= p["theta"] and ec >= p["theta"]):
        fails.append("floor")
    twist = ec <= F32(p["tau"] * er) and (wrong == "twist_one_sided" or er <= F32(p["tau"] * ec))
    if not twist:
        fails.append("twist")
    dom = all(j == r or rows[j] <= F32(p["delta"] * rows[r]) for j in range(4)) and \
        all(j == c or cols[j] <= F32(p["delta"] * cols[c]) for j in range(4))
    if not dom:
        fails.append("dominance")
    pair_sum = F32(rows[r] + cols[c]) if wrong == "purity_on_P" else F32(er + ec)
    if not pair_sum >= F32(p["pi2"] * Ex):
        fails.append("purity")
    if not fails:
        tr.add("pair")
        return 1 + 4 * r + c
    tr.add("pair_fails_" + fails[0] + ("_alone" if len(fails) == 1 else "_with_others"))
    if p["singles"] != 0:
        need = F32(p["pi1"] * Ex)
        for k, code in ((8, 17), (9, 18)):
            if e[k] >= p["theta"] and e[k] >= need:
                tr.add("single")
                return code
    else:
        tr.add("singles_off")
    tr.add("none")
    return 0


def decide(p, rec, Ex, P, tr, wrong=None):
    """Steps 3 .. 5: the record (8 float32, words 6 and 7 untouched) after the block."""
    tone, cand0, run, hold, guard, events = (F32(v) for v in rec[:6])
    cand = F32(candidate(p, Ex, P, tr, wrong))
    if cand != 0 and cand == cand0:
        run = F32(run + F32(1))
        tr.add("run_continues")
    else:
        if cand != 0 and cand0 != 0:
            tr.add("run_broken_by_other")
        run = F32(1) if cand != 0 else F32(0)
    need_g = p["G"] if cand < 17 else p["N1"]
    need_r = p["N2"] if cand < 17 else p["N1"]
    if cand != 0 and run >= need_g:
        guard, hold = F32(1), p["H"]
        tr.add("guard_candidate")
        if wrong == "hold_on_candidate" and hold > 0:
            hold = F32(hold - F32(1))
    elif hold > 0:
        hold, guard = F32(hold - F32(1)), F32(1)
        tr.add("guard_hold")
        if tone != 0:
            tr.add("tone_kept_in_hold")
    else:
        guard = F32(0)
        tr.add("unguarded")
        if cand != 0:
            tr.add("candidate_waits")
    if cand != 0 and run >= need_r:
        if tone != cand or wrong == "events_every_block":
            events = F32(events + F32(1))
            tr.add("event")
        else:
            tr.add("event_continues")
        tone = cand
        tr.add("reported")
    elif guard == 0:
        tone = F32(0)
    out = np.array(rec, np.float32).reshape(8)
    out[:6] = [tone, cand, run, hold, guard, events]
    return out


def block(p16, tab, record, x, wrong=None, sums=None):
    """Steps 1 and 3 .. 5 of one block that is not a structural zero -> (the record, guarded?, the trace).  sums: (E_x, P) of
    the block where the caller has them already."""
    assert wrong is None or wrong in WRONG, wrong
    p = dict(zip(NAMES, np.asarray(p16, np.float32)[:11]))
    tr = set()
    Ex, P = powers(np.asarray(x, np.float32).reshape(256), tab, wrong == "pairwise") if sums is None else sums
    rec = decide(p, np.asarray(record, np.float32).reshape(8), Ex, P, tr, wrong)
    return rec, bool(p["mode"] == 1 and rec[4] == 1), tr


def detect(p16, tab, x, record=None, wrong=None):
    """Steps 1 .. 5 and 7 over the blocks of x (256 K,), none of them a structural zero -> records (K, 8), traces."""
    rec = np.zeros(8, np.float32) if record is None else np.array(record, np.float32)
    xb = np.asarray(x, np.float32).reshape(-1, 256)
    Ex, P = powers(xb, tab, wrong == "pairwise")
    recs, traces = [], []
    for k in range(len(xb)):
        rec, _, tr = block(p16, tab, rec, xb[k], wrong, (Ex[k], P[k]))
        rec[6], rec[7] = F32(rec[6] + rec[4]), F32(rec[7] + F32(1))
        recs.append(rec.copy())
        traces.append(tr)
    return np.stack(recs), traces


def stream(p16, tab, w, x, gain=None, ramp_word=None, alc_params=None, first_block_index=0, record=None, alc_record=None,
           meters=None):
    """One stream through steps 1 .. 7.  w, x: (K, 256) blocks in hop order; p16: 16 words, or one set per block; gain: None,
    a number or one per block; ramp_word: None (no ramps) or the word in front of the first block.  Returns a dict: y (K, 256),
    records (K, 8), traces, ramp words (K,), alc records (K, 8) and meter records (K, 4) after every block."""
    w, x = (np.asarray(v, np.float32).reshape(-1, 256) for v in (w, x))
    K = len(w)
    p16 = np.asarray(p16, np.float32)
    gains = None if gain is None else np.broadcast_to(np.asarray(gain, np.float32), (K,))
    rec = np.zeros(8, np.float32) if record is None else np.array(record, np.float32)
    arec = AK.INIT.copy() if alc_record is None else np.array(alc_record, np.float32)
    mrec = None if meters is None else np.array(meters, np.float32)
    pw = None if ramp_word is None or gains is None else F32(ramp_word)
    out = dict(y=[], records=[], traces=[], ramp=[], alc=[], meters=[], m=[])
    for k in range(K):
        pk16 = p16 if p16.ndim == 1 else p16[k]
        g = None if gains is None else F32(gains[k])
        if first_block_index + k == 0:
            y = m = np.zeros(256, np.float32)
            rec, tr = np.zeros(8, np.float32), {"zero"}
            arec = AK.INIT.copy()
            ex = F32(0)
            if pw is not None:
                pw = g
        else:
            rec, dry, tr = block(pk16, tab, rec, x[k])
            rec[6], rec[7] = F32(rec[6] + rec[4]), F32(rec[7] + F32(1))
            if dry:
                tr.add("passed_dry")
                m = RK.mix(F32(1), x[k], w[k]) if g is not None else x[k].copy()
                if pw is not None:
                    pw = F32(1)
            elif g is not None:
                if pw is not None and pw != g:
                    tr.add("ramps_from_1" if pw == 1 else "ramps")
                    m, pw = RK.mix(RK.ramp(pw, g), x[k], w[k]), g
                else:
                    m = RK.mix(g, x[k], w[k])
            else:
                m = w[k].copy()
            y = m
            if alc_params is not None:
                y, arec, atr, _ = AK.block(alc_params, arec, w[k], x[k], m)
                tr |= {"alc_" + t for t in atr}
            ex = AK.hop_sum(x[k])
        if mrec is not None:
            with np.errstate(all="ignore"):
                mrec = np.array([F32(mrec[0] + ex), F32(mrec[1] + AK.hop_sum(y)),
                                 np.fmax(mrec[2], np.fmax.reduce(np.abs(y), initial=F32(0))), F32(mrec[3] + F32(1))], np.float32)
        for key, v in (("y", y), ("records", rec.copy()), ("traces", tr), ("ramp", pw), ("alc", arec.copy()), ("meters", mrec),
                       ("m", m)):
            out[key].append(v)
    for key in ("y", "records", "alc", "m"):
        out[key] = np.stack(out[key])
    return out


def seen(traces):
    out = set()
    for t in traces:
        out |= t
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


# ---- signals of the behaviour gate
def dtmf(code, n, start, amp=0.1, total=None, df=0.0, twist_db=0.0, phase=0.0):
    """A digit (code 1 .. 16) of n samples at 16 kHz starting at sample `start` of a buffer of `total` samples: amp per tone,
    the column tone raised / the row tone lowered by twist_db / 2 each, both frequencies off by the factor 1 + df."""
    total = start + n if total is None else total
    r, c = divmod(code - 1, 4)
    t = np.arange(n) / 16000.0
    a = amp * 10 ** (-twist_db / 40), amp * 10 ** (twist_db / 40)
    s = a[0] * np.sin(2 * np.pi * FREQS[r] * (1 + df) * t + phase) + a[1] * np.sin(2 * np.pi * FREQS[4 + c] * (1 + df) * t + 2 * phase)
    out = np.zeros(total)
    out[start:start + n] = s
    return out


def reported_codes(records):
    """The onsets a record sequence reports: the tone codes at the blocks where `events` rose."""
    ev = np.concatenate([[0], records[:, 5]])
    return [int(records[k, 0]) for k in range(len(records)) if ev[k + 1] > ev[k]]
