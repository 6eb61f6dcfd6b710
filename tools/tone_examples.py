#!/usr/bin/env python3
"""What the tone guard's detector does on real audio and on short digits (a report; tests/test_tone_host.py holds the gate).

Through the contract's numpy float32 statement (tests/tone_checker.py) with the defaults, no GPU:
  - the five noisy rows of tests/golden/examples_full.npz (1 937 blocks each): reported events, candidate blocks and guarded
    blocks per clip;
  - all 16 digits at the 16 start offsets 0, 16, .., 240 within a block, amplitude 0.1 per tone: how many of the 256 are
    reported at 20, 23, 30 and 40 ms, at +-1.5 % and +-3.5 % frequency offset, at +-6 dB twist and in white noise at 15, 10
    and 5 dB SNR, with the number of wrong digits.

    python tools/tone_examples.py [--out profiles/tone_examples.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def digits(TK, tab, n, rng=None, snr_db=None, **kw):
    p, found, wrong = TK.params(), 0, 0
    for code in range(1, 17):
        for off in range(0, 256, 16):
            total = 256 * (3 + -(-n // 256))
            x = TK.dtmf(code, n, 256 + off, total=total, **kw)
            if snr_db is not None:
                x = x + math.sqrt(0.01 / 10 ** (snr_db / 10)) * rng.standard_normal(total)
            codes = TK.reported_codes(TK.detect(p, tab, x.astype(np.float32))[0])
            found += code in codes
            wrong += any(c != code for c in codes)
    return {"reported": found, "of": 256, "wrong": wrong}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tone_examples.json"))
    a = ap.parse_args(argv)
    import tone_checker as TK
    tab = TK.table()
    res = {"arithmetic": "numpy float32, tests/tone_checker.py", "defaults": TK.DEFAULTS, "clips": [], "digits": {}}
    noisy = np.load(os.path.join(ROOT, "tests", "golden", "examples_full.npz"))["noisy"]
    for i, row in enumerate(noisy):
        x = (row[:256 * (len(row) // 256)].astype(np.float32) / np.float32(32768)).astype(np.float32)
        recs, _ = TK.detect(TK.params(), tab, x)
        res["clips"].append({"clip": i, "blocks": len(recs), "events": int(recs[-1, 5]), "candidate_blocks": int((recs[:, 1] != 0).sum()),
                             "guarded_blocks": int(recs[-1, 6])})
    rng = np.random.default_rng(74)
    for ms in (20, 23, 30, 40):
        res["digits"]["%d ms" % ms] = digits(TK, tab, 16 * ms)
    for df in (-0.035, -0.015, 0.015, 0.035):
        res["digits"]["40 ms, frequency %+.1f %%" % (100 * df)] = digits(TK, tab, 640, df=df)
    for tw in (-6.0, 6.0):
        res["digits"]["40 ms, twist %+.0f dB" % tw] = digits(TK, tab, 640, twist_db=tw)
    for snr in (15.0, 10.0, 5.0):
        res["digits"]["40 ms, white noise at %.0f dB SNR" % snr] = digits(TK, tab, 640, rng, snr_db=snr)
    json.dump(res, open(a.out, "w"), indent=1)
    for c in res["clips"]:
        print(c)
    for k, v in res["digits"].items():
        print(k, v)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
