#!/usr/bin/env python3
"""The reference's own SDR / SI-SNR numbers for the pairs the score tests use.

Run only in the build container (the reference does not travel to the GPU box):

    PYTHONPATH=/root/reference PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_score.py

Imports eval/eval_intrusive_metrics.py with its missing imports stubbed (librosa, soundfile, p_tqdm, pesq, pystoi: none
of them is used by sisnr_metric / sdr_metric) and calls those two functions on float32 pairs:
  * the 15 four-second excerpts of examples_full.npz (enhanced against noisy, offsets 0 / 8 / 16 s), and
  * a speech excerpt against itself plus white noise at -5 .. 30 dB SNR (tests/score_checker.py:ladder_pair).
Writes score_ref.npz: excerpt indices, SNRs and the returned numbers only (a few KB), and MANIFEST_score.json with
max |reference float32 - checker float64| per metric: the reference's own noise floor, which the GPU test's comparison
with these numbers is held to.
"""
import json
import os
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))
for name in ("librosa", "soundfile", "p_tqdm", "pesq", "pystoi"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["p_tqdm"].p_map = None
sys.modules["pesq"].PesqError = None
sys.modules["pesq"].pesq = None
sys.modules["pystoi"].stoi = None

from gtcrn_micro.eval.eval_intrusive_metrics import sdr_metric, sisnr_metric  # noqa: E402

import score_checker as SC  # noqa: E402


def main():
    ex = np.load(os.path.join(HERE, "examples_full.npz"))
    pairs = [SC.excerpt_pair(ex, c, o) for c, o in SC.EXCERPTS] + [SC.ladder_pair(ex, s) for s in SC.SNR_LADDER]
    sdr = np.array([float(sdr_metric(r, y)) for r, y in pairs])
    sisnr = np.array([float(sisnr_metric(r, y)) for r, y in pairs])
    for r, y in pairs:
        assert r.dtype == np.float32 and y.dtype == np.float32
    c_sdr = np.array([SC.sdr(r, y) for r, y in pairs])
    c_sisnr = np.array([SC.sisnr(r, y) for r, y in pairs])
    np.savez(os.path.join(HERE, "score_ref.npz"), excerpts=np.array(SC.EXCERPTS, np.int32),
             snr_ladder=np.array(SC.SNR_LADDER), sdr=sdr, sisnr=sisnr)
    meta = {"numpy": np.__version__, "pairs": len(pairs),
            "sdr_reference_float32_vs_checker_float64_max_db": float(np.abs(sdr - c_sdr).max()),
            "sisnr_reference_float32_vs_checker_float64_max_db": float(np.abs(sisnr - c_sisnr).max())}
    json.dump(meta, open(os.path.join(HERE, "MANIFEST_score.json"), "w"), indent=1)
    print(json.dumps(meta, indent=1))
    print("sdr", np.round(sdr, 4))
    print("sisnr", np.round(sisnr, 4))


if __name__ == "__main__":
    main()
