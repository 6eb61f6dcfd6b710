#!/usr/bin/env python3
"""Measures max |gpu - float64 checker| per quantity over the inputs of tests/test_gpu_score.py on the GPU at hand and
writes profiles/score_parity.json, the file that test takes its tolerances from (4 x each figure).  Run it on an MI355X
after a change of kernels, compiler or box, look at what moved, and commit the file with the change.

    python tools/score_parity.py [--out profiles/score_parity.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_parity.json"))
    a = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "score_parity needs the GPU"
    import score_checker as SC
    import test_gpu_score as T
    from gtcrn_micro_amd import Scorer
    sc = Scorer(0)
    worst = T.measure(sc)
    bad = 0
    for name in SC.GPU_CASES:
        g = T.gpu_case(sc, name)
        for b, sp in enumerate(g["specs"]):
            want = SC.case_reference(sp)
            bad += not (tuple(g["counts"][b]) == (want["kept_frames"], want["segments"])
                        and (g["hooks"][b][2] != 0).tolist() == want["stages"]["mask"].tolist())
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "what": "max |gpu - float64 checker| over the inputs of tests/test_gpu_score.py (measure()): every clip of "
                   "tests/score_checker.py:GPU_CASES, a signal against itself, the silent pairs and the synthetic_mix "
                   "clips of the score_batch test; x10 and env relative to the clip's peak, energies in dB, sdr / sisnr "
                   "in dB, stoi absolute; stoi_synthetic_mix is STOI of the synthetic_mix clips alone (a reference with "
                   "empty third-octave bands) and is not part of stoi",
           "clips": sum(len(c) for _, c in SC.GPU_CASES.values()) + 1 + 3 + 3, "mask_or_count_mismatches": int(bad),
           "measured": worst}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res, indent=1))
    sc.close()


if __name__ == "__main__":
    main()
