#!/usr/bin/env python3
"""How the level control behaves on real audio (a report, not a gate): the five example pairs of
tests/golden/examples_full.npz through the hop form with the trained parameters and the defaults (alc=True).

The fixture holds each noisy file and the reference implementation's enhanced file of it; no studio-clean file exists, so the
enhanced file of the pair stands in for the clean one.  Its activity is DESIGN 7o's: windows of 1600 samples, active iff the
sum of squares of the int16 samples exceeds floor(2^30 * 10^(-50 / 10)) times the window length.  An emitted block counts as
active when more than half of its 256 samples lie in active windows (block k lies over input hop k - 1).
Per clip: the agreement of `voice` with that activity, the output's level over the voiced blocks against the target, and
the number of blocks the limiter touched -- read from the trace of the contract's numpy statement (tests/alc_checker.py) run
on the blocks of a twin state without level control, which must also reproduce the device's records bit for bit.

    python tools/alc_examples.py [--out profiles/alc_examples.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


VARIANTS = {"floor -55": dict(floor_dbov=-55), "floor -50": dict(floor_dbov=-50), "floor -40": dict(floor_dbov=-40),
            "hang 100 ms": dict(hang_ms=100), "floor -55, hang 100 ms": dict(floor_dbov=-55, hang_ms=100),
            "ratio -6": dict(ratio_db=-6)}


def block_activity(pcm, nblocks, window=1600, db=-50.0):
    thr = int(np.floor(2.0 ** 30 * 10.0 ** (db / 10.0)))
    x = pcm.astype(np.int64)
    act = np.zeros(len(x), bool)
    for lo in range(0, len(x), window):
        seg = x[lo:lo + window]
        act[lo:lo + window] = int((seg * seg).sum()) > thr * len(seg)
    out = np.zeros(nblocks, bool)
    for k in range(1, nblocks):
        seg = act[256 * (k - 1):256 * k]
        out[k] = len(seg) > 0 and seg.mean() > 0.5
    return out


def dbov(e, n):
    return float(10.0 * np.log10(e / n)) if n and e > 0 else None


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alc_examples.json"))
    a = ap.parse_args(argv)
    import torch
    import alc_checker as AK
    from gtcrn_micro_amd import Engine, make_window, alc_params, _lib
    assert torch.cuda.is_available(), "alc_examples needs the GPU"
    params = np.fromfile(os.path.join(ROOT, "tests", "golden", "params_dns3.f32"), dtype=np.float32)
    ex = np.load(os.path.join(ROOT, "tests", "golden", "examples_full.npz"))
    eng = Engine(params, 0)
    win = torch.from_numpy(make_window(0)).cuda()
    noisy = torch.from_numpy(ex["noisy"].astype(np.float32) / 32768.0).cuda()
    N, K = noisy.shape[0], noisy.shape[1] // 256
    st, plain = eng.new_wave_state(N, win, alc=True), eng.new_wave_state(N, win)
    ys, ws, recs = [], [], []
    for k in range(K):
        hop = noisy[:, 256 * k:256 * (k + 1)]
        ys.append(eng.wave_stream_step(st, hop))
        ws.append(eng.wave_stream_step(plain, hop))
        recs.append(st.alc.clone())
    y, w = torch.stack(ys, 1).cpu().numpy(), torch.stack(ws, 1).cpu().numpy()      # (N, K, 256)
    rec = torch.stack(recs, 1).cpu().numpy()                                     # (N, K, 8)
    x = np.concatenate([np.zeros((N, 1, 256), np.float32), noisy.cpu().numpy()[:, :256 * (K - 1)].reshape(N, K - 1, 256)], 1)
    words = alc_params()
    res = {"device": torch.cuda.get_device_name(0), "settings": dict(_lib.ALC_DEFAULTS), "blocks_per_clip": K,
           "activity": "the reference's enhanced file of each pair, DESIGN 7o's windows (1600 samples, -50 dB)", "clips": []}
    for s in range(N):
        yc, rc, traces = AK.stream(words, w[s], x[s], w[s])
        exact = bool(AK.same_bits(yc, y[s]) and AK.same_bits(rc, rec[s]))
        voice = rec[s, :, 3] != 0
        active = block_activity(ex["enh"][s], K)
        limited = np.array(["limited" in t for t in traces])
        e_out = (y[s].astype(np.float64) ** 2).sum(1)
        e_wet = (w[s].astype(np.float64) ** 2).sum(1)
        gain_db = 20.0 * np.log10(rec[s, :, 0].astype(np.float64))
        row = {"checker_reproduces_device_bits": exact,
               "agreement": float((voice == active).mean()),
               "active_share": float(active.mean()), "voice_share": float(voice.mean()),
               "voice_given_active": float(voice[active].mean()) if active.any() else None,
               "voice_given_inactive": float(voice[~active].mean()) if (~active).any() else None,
               "target_dbov": _lib.ALC_DEFAULTS["target_dbov"],
               "output_level_over_voiced_blocks_dbov": dbov(e_out[voice].sum(), 256 * int(voice.sum())),
               "wet_level_over_voiced_blocks_dbov": dbov(e_wet[voice].sum(), 256 * int(voice.sum())),
               "output_level_over_last_half_voiced_dbov": dbov(e_out[K // 2:][voice[K // 2:]].sum(), 256 * int(voice[K // 2:].sum())),
               "gain_db_end": float(gain_db[-1]), "gain_db_min": float(gain_db.min()), "gain_db_max": float(gain_db.max()),
               "limiter_blocks": int(limited.sum()), "output_peak": float(np.abs(y[s]).max())}
        # the same blocks through the numpy statement with other settings (host only): what a default could be traded for
        row["variants"] = {}
        for name, kw in VARIANTS.items():
            _, rv, _ = AK.stream(alc_params(**kw), w[s], x[s], w[s])
            vv = rv[:, 3] != 0
            row["variants"][name] = {"agreement": float((vv == active).mean()),
                                     "voice_given_active": float(vv[active].mean()) if active.any() else None,
                                     "voice_given_inactive": float(vv[~active].mean()) if (~active).any() else None}
        res["clips"].append(row)
        print("clip %d: agreement %.3f (voice | active %.3f, voice | inactive %.3f), output %.1f dBov over voiced blocks (wet %.1f, "
              "target %.0f), gain %.1f .. %.1f dB, %d limiter blocks, bits %s" % (
                  s, row["agreement"], row["voice_given_active"] or 0, row["voice_given_inactive"] or 0,
                  row["output_level_over_voiced_blocks_dbov"] or 0, row["wet_level_over_voiced_blocks_dbov"] or 0,
                  row["target_dbov"], row["gain_db_min"], row["gain_db_max"], row["limiter_blocks"], exact), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
