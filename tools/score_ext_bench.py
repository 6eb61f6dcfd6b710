#!/usr/bin/env python3
"""What ESTOI and segmental SNR cost next to the three scores they join (not a gate; bench.py is untouched).

For B = 256 and B = 8 clips of 4 s, in one process, by the method of tools/score_bench.py (warmed, medians over windows
of back-to-back calls, device events): all five metrics through Scorer.score_ext, the three old ones through
Scorer.score, each new metric alone, the ratio of the two full calls, and each launch's time in a score_ext call
(gtcrn_score_timing: events around the nine launches).

    python tools/score_ext_bench.py [--out profiles/score_ext_bench.json] [--iters 200]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_ext_bench.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--seconds", type=float, default=4.0)
    a = ap.parse_args(argv)
    import torch
    from gtcrn_micro_amd import Scorer
    import score_checker as SC
    from score_bench import median_ms
    assert torch.cuda.is_available(), "score_ext_bench needs the GPU"
    sc = Scorer(0)
    L = int(a.seconds * 16000)
    ex = SC.examples()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "clip_seconds": a.seconds,
           "timing": "median (min, max) over %d windows of 10 calls, device events, after 20 warm-up calls" % a.iters,
           "pairs": "(noisy, enhanced) excerpts of tests/golden/examples_full.npz", "batches": {}}
    for B in (256, 8):
        starts = [(k * 7919) % (ex["noisy"].shape[1] - L) for k in range(B)]
        cut = lambda key: torch.from_numpy(np.stack([ex[key][k % 5, s:s + L] for k, s in enumerate(starts)]).astype(np.float32)
                                           / 32768.0).cuda()
        ref, y = cut("noisy"), cut("enh")
        rec, rec8 = torch.empty((B, 4), device="cuda", dtype=torch.float64), torch.empty((B, 8), device="cuda", dtype=torch.float64)
        row = {"score_ext_all_five_ms": median_ms(lambda: sc.score_ext(ref, y, out=rec8), a.iters),
               "score_three_ms": median_ms(lambda: sc.score(ref, y, out=rec), a.iters),
               "score_ext_three_ms": median_ms(lambda: sc.score_ext(ref, y, what=("sdr", "sisnr", "stoi"), out=rec8), a.iters),
               "score_ext_estoi_alone_ms": median_ms(lambda: sc.score_ext(ref, y, what=("estoi",), out=rec8), a.iters),
               "score_ext_segsnr_alone_ms": median_ms(lambda: sc.score_ext(ref, y, what=("segsnr",), out=rec8), a.iters)}
        row["ext_over_three"] = row["score_ext_all_five_ms"][0] / row["score_three_ms"][0]
        sc.timing(True)
        stages = {}
        for _ in range(50):
            sc.score_ext(ref, y, out=rec8)
            for name, ms in sc.ext_timing_read().items():
                stages.setdefault(name, []).append(ms)
        sc.timing(False)
        med = {k: statistics.median(v) for k, v in stages.items()}
        tot = sum(med.values())
        row["launch_ms"] = med
        row["launch_share"] = {k: v / tot for k, v in med.items()}
        row["segsnr_bytes_read_once"] = 2 * 4 * B * L
        row["mean_estoi"] = float(rec8[:, 4].mean())
        row["mean_segsnr_db"] = float(rec8[:, 5].mean())
        res["batches"][f"B{B}"] = row
        print(f"B={B}: score_ext (five) {row['score_ext_all_five_ms'][0]:.4f} ms, score (three) {row['score_three_ms'][0]:.4f} ms "
              f"(x{row['ext_over_three']:.2f}); launches " + ", ".join(f"{k} {v * 1e3:.1f} us" for k, v in med.items()), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
