#!/usr/bin/env python3
"""Measures max |gpu - float64 checker| of ESTOI and segmental SNR over the inputs of tests/test_gpu_score_ext.py on the
GPU at hand and writes profiles/score_ext_parity.json, the file that test takes its tolerances from (4 x each figure).
Run it on an MI355X after a change of kernels, compiler or box, look at what moved, and commit the file with the change.

    python tools/score_ext_parity.py [--out profiles/score_ext_parity.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_ext_parity.json"))
    a = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "score_ext_parity needs the GPU"
    import score_checker as SC
    import score_ext_checker as SX
    import test_gpu_score_ext as T
    from gtcrn_micro_amd import Scorer
    sc = Scorer(0)
    worst = T.measure(sc)
    bad = 0
    for name in T.PARITY_CASES:
        g = T.gpu_case(sc, name)
        for b, sp in enumerate(g["specs"]):
            want = SX.case_reference(sp)
            bad += (g["kept"][b], g["segs"][b], g["frames"][b]) != (want["kept_frames"], want["segments"], want["segsnr_frames"])
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "what": "max |gpu - float64 checker| over the checker comparisons of tests/test_gpu_score_ext.py (measure()): the "
                   "clips of tests/score_checker.py:GPU_CASES " + ", ".join(T.PARITY_CASES) + ", the segment-edge and "
                   "frame-edge batches, a signal against itself and the silent pairs; estoi absolute, segsnr_db in dB",
           "clips": sum(len(SC.GPU_CASES[n][1]) for n in T.PARITY_CASES) + 6 + 126 + 1 + 3, "count_mismatches": int(bad),
           "measured": worst}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res, indent=1))
    sc.close()


if __name__ == "__main__":
    main()
