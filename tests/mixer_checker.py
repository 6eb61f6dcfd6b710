"""The conference mix (include/gtcrn_micro_hip.h, "conference rooms") restated in numpy float32: steps 1 - 9, every
operation one rounded float32 operation, in the contract's order.  Independent of csrc/."""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(F).max
MAX_ROOM = 1024


def params(k=3, floor_dbov=-50.0, alpha=0.125, incumbent_db=3.0):
    return np.array([k, 10.0 ** (floor_dbov / 10.0), alpha, 10.0 ** (incumbent_db / 10.0), 0, 0, 0, 0], np.float64).astype(F)


def energy(s):
    """Step 1: 64 lanes of strided sums of rounded squares, then the xor butterfly."""
    v = np.zeros(64, F)
    for j in range(0, len(s), 64):
        c = s[j:j + 64]
        v[:len(c)] = v[:len(c)] + c * c
    for d in (1, 2, 4, 8, 16, 32):
        v = v + v[np.arange(64) ^ d]
    return v[0]


def mix(x, out, room_start, seats, rec, prm, nrooms=None, voice=None, vstride=1):
    """x (n_in, n) float32 or int16; out (n_out, n) of the same type and rec (n_rec, 4) float32 are written in place."""
    pcm, n = x.dtype == np.int16, x.shape[1]
    K, theta, alpha, kappa = int(prm[0]), F(prm[1]) * F(n), F(prm[2]), F(prm[3])
    ramp = np.arange(1, n + 1).astype(F) / F(n)
    R = len(room_start) - 1 if nrooms is None else max(0, min(int(nrooms), len(room_start) - 1))
    with np.errstate(all="ignore"):
        for r in range(R):
            a, b = int(room_start[r]), int(room_start[r + 1])
            if a < 0 or b < a or b > len(seats) or b - a > MAX_ROOM:
                continue
            room = []                                     # per seat: [in_row, out_row, rec, s, present, g_old, key, t]
            for i, o, q, _ in seats[a:b]:
                if not 0 <= q < len(rec):
                    continue
                s = None
                if 0 <= i < len(x):
                    s = x[i].astype(F) / F(32768) if pcm else x[i].astype(F)
                E = energy(s) if s is not None else F(0)
                present = s is not None and bool(E <= FLT_MAX)
                key = F(-1)
                if present:                               # steps 3 - 5
                    lv = rec[q, 1]
                    rec[q, 1] = E if E >= lv else lv + alpha * (E - lv)
                    eligible = voice[q * vstride] != 0 if voice is not None else E >= theta
                    if eligible:
                        key = kappa * rec[q, 1] if rec[q, 0] == 1 else rec[q, 1]
                room.append([i, o if 0 <= o < len(out) else -1, q, s, present, int(present and rec[q, 0] == 1), key, 0])
            for _ in range(K):                            # step 6: strict >, so a tie stays with the lower seat
                best = None
                for p, st in enumerate(room):
                    if not st[7] and st[6] > 0 and (best is None or st[6] > room[best][6]):
                        best = p
                if best is None:
                    break
                room[best][7] = 1
            staged = {}                                   # step 7: the gained blocks of the contributors, in seat order
            for p, (i, o, q, s, present, g, key, t) in enumerate(room):
                if present and g + t > 0:
                    gain = np.ones(n, F) if g and t else (ramp if t else F(1) - ramp)
                    staged[p] = gain * s
            for p, (i, o, q, s, present, g, key, t) in enumerate(room):
                if o >= 0:                                # step 8
                    acc = np.zeros(n, F)
                    for c, block in staged.items():
                        if c != p:
                            acc = acc + block
                    out[o] = np.clip(np.rint(F(32768) * acc), -32768, 32767).astype(np.int16) if pcm else acc
                rec[q] = [t if present else 0, rec[q, 1], rec[q, 2] + F(t), rec[q, 3] + F(1)]   # step 9


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
