"""Checker of the level control (include/gtcrn_micro_hip.h, "level control"): steps 1 .. 11 of the contract in numpy float32,
every operation one rounding, the reductions in the stated order.  It reproduces a device output and a device record bit for
bit from the blocks the calls WITHOUT level control emit: w (wet), x (the dry samples under them) and m (what the call would
store: w, or the mix with gains).

`block` advances one record by one block and returns the names of the branches it took (the trace); `stream` runs the blocks
of one stream, the structural zero of step 2 included.  `wrong=` distorts one definition at a time: the seeded bugs the
comparison must reject."""
import numpy as np

import ramp_checker as RK

F32 = np.float32
FMAX = F32(np.finfo(np.float32).max)
INIT = np.array([1, 0, 0, 0, 0, 0, 0, 0], np.float32)
WRONG = ("hang_moves_S", "limit_a1_only", "ew_after_mix", "ratio_prev_ew", "pairwise")
NAMES = ("theta", "rho", "H", "alpha", "T", "a_min", "a_max", "d_up", "d_dn", "c", "mode")


def hop_sum(block, pairwise=False):
    """Step 1's order: lane l holds samples 2l, 2l+1, 128+2l, 129+2l, p = ((s0^2 + s1^2) + s2^2) + s3^2, then the xor
    butterfly over lane distances 1 .. 32.  (tests/meter_checker.py's hop_sum, without its assertion on NaN payloads.)"""
    b = np.asarray(block, np.float32)
    with np.errstate(all="ignore"):
        sq = (b * b).astype(np.float32)
        if pairwise:                                      # the seeded bug: numpy's own pairwise sum
            return F32(np.sum(sq, dtype=np.float32))
        lane = np.arange(64)
        p = (sq[2 * lane] + sq[2 * lane + 1]).astype(np.float32)
        p = (p + sq[128 + 2 * lane]).astype(np.float32)
        p = (p + sq[129 + 2 * lane]).astype(np.float32)
        for d in (1, 2, 4, 8, 16, 32):
            p = (p + p[lane ^ d]).astype(np.float32)
    return p[0]


def block(params, record, w, x, m, wrong=None, prev_ew=None):
    """One emitted block that is not a structural zero -> (y, the record after it, the trace, E_w)."""
    assert wrong is None or wrong in WRONG, wrong
    P = dict(zip(NAMES, np.asarray(params, np.float32)[:11]))
    w, x, m = (np.asarray(v, np.float32).reshape(256) for v in (w, x, m))
    rec = np.array(record, np.float32).reshape(8)
    a, S, hang = rec[0], rec[1], rec[2]
    tr = set()
    with np.errstate(all="ignore"):
        Ew = hop_sum(m if wrong == "ew_after_mix" else w, wrong == "pairwise")
        Ex = hop_sum(x, wrong == "pairwise")
        pk = F32(np.fmax.reduce(np.abs(m), initial=F32(0)))
        at, voice, a0, a1 = a, F32(0), a, a
        if not (Ew <= FMAX and Ex <= FMAX and pk <= FMAX):
            tr.add("nonfinite")
            for name, v in (("Ew", Ew), ("Ex", Ex), ("pk", pk)):      # which reduction, and of what kind
                if not v <= FMAX:
                    tr.add(name + ("_nan" if np.isnan(v) else "_inf"))
        else:
            rx = F32(P["rho"] * Ex)
            ratio_of = prev_ew if wrong == "ratio_prev_ew" and prev_ew is not None else Ew
            speech = bool(Ew >= P["theta"] and ratio_of >= rx)
            if Ew == P["theta"]:
                tr.add("tie_theta")
            if Ew == rx and Ew > 0:
                tr.add("tie_ratio")
            moves_S = speech
            if speech:
                hang, voice = P["H"], F32(1)
                tr.add("speech")
            elif hang > 0:
                hang, voice = F32(hang - F32(1)), F32(1)
                tr.add("hangover")
                if hang == 0:
                    tr.add("hangover_ends")
                moves_S = wrong == "hang_moves_S"
            else:
                tr.add("silence")
            if moves_S:
                if S == 0:
                    S = Ew
                    tr.add("first_estimate")
                else:
                    S = F32(S + F32(P["alpha"] * F32(Ew - S)))
                    tr.add("smoothed")
            if voice and S > 0:
                root = np.sqrt(F32(P["T"] / S))
                tr.add("clamp_a_min" if root < P["a_min"] else "clamp_a_max" if root > P["a_max"] else "inside_range")
                want = min(max(root, P["a_min"]), P["a_max"])
                lo, hi = F32(a * P["d_dn"]), F32(a * P["d_up"])
                tr.add("fall_limited" if want < lo else "rise_limited" if want > hi else "reached")
                at = min(max(want, lo), hi)
            a0, a1 = a, at
            if pk == 0:
                tr.add("pk_zero")
            if pk > 0 and F32(pk * max(a, at)) > P["c"]:
                q = F32(P["c"] / pk)
                L = max(P["a_min"], q)
                if q < P["a_min"]:
                    tr.add("limiter_at_a_min")
                a0 = a if wrong == "limit_a1_only" else min(a, L)
                a1 = min(at, L)
                tr.add("limited")
                tr.add("limited_both" if L < at else "limited_start_only" if L < a else "limited_neither")
            else:
                tr.add("unlimited")
        if P["mode"] == 0:
            a0 = a1 = F32(1)
            tr.add("mode0")
        y = (RK.ramp(a0, a1) * m).astype(np.float32)
        rec[:6] = [a1, S, hang, voice, F32(rec[4] + voice), F32(rec[5] + F32(1))]
    return y, rec, tr, Ew


def stream(params, w, x, m, first_block_index=0, record=None, wrong=None):
    """One stream.  w, x, m: (K, 256) blocks in hop order; params: 16 words, or one set of them per block; the stream's first
    block here is block `first_block_index` of its life (block 0 is the structural zero: zeros out, the record becomes INIT).
    Returns y (K, 256), the records after every block (K, 8) and the list of traces."""
    w, x, m = (np.asarray(v, np.float32).reshape(-1, 256) for v in (w, x, m))
    params = np.asarray(params, np.float32)
    rec = INIT.copy() if record is None else np.array(record, np.float32).reshape(8)
    ys, recs, traces, prev = [], [], [], None
    for k in range(len(w)):
        if first_block_index + k == 0:
            y, rec, tr = np.zeros(256, np.float32), INIT.copy(), {"zero"}
        else:
            y, rec, tr, prev = block(params if params.ndim == 1 else params[k], rec, w[k], x[k], m[k], wrong, prev)
        ys.append(y)
        recs.append(rec.copy())
        traces.append(tr)
    return np.stack(ys), np.stack(recs), traces


def seen(traces):
    out = set()
    for t in traces:
        out |= t
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())
