#!/usr/bin/env python3
"""What scoring costs next to the enhancement it scores (not a gate; bench.py is untouched).

For B = 256 and B = 8 clips of 4 s: warmed medians of Scorer.score (all three metrics, and SDR + SI-SNR alone) and of
Engine.forward_wave on the same batch in the same process, the ratio score / enhance, each launch's share of a scoring
call (gtcrn_score_timing: events around the six launches), and -- as CPU context -- the time the float64 checker
(tests/score_checker.py; our checker, not pystoi) takes per clip on this host.

    python tools/score_bench.py [--out profiles/score_bench.json] [--iters 200]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_ms(fn, iters, warmup=20, per=10):
    """Median over `iters` windows of `per` back-to-back calls each, timed with device events."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / per)
    return statistics.median(out), min(out), max(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--seconds", type=float, default=4.0)
    a = ap.parse_args(argv)
    import torch
    from gtcrn_micro_amd import Engine, Scorer, make_window
    import score_checker as SC
    assert torch.cuda.is_available(), "score_bench needs the GPU"
    params = np.fromfile(os.path.join(ROOT, "tests", "golden", "params_dns3.f32"), dtype=np.float32)
    eng, sc = Engine(params, 0), Scorer(0)
    win = torch.from_numpy(make_window(0)).cuda()
    L = int(a.seconds * 16000)
    ex = SC.examples()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "clip_seconds": a.seconds,
           "timing": "median (min, max) over %d windows of 10 calls, device events, after 20 warm-up calls" % a.iters,
           "batches": {}}
    for B in (256, 8):
        starts = [(k * 7919) % (ex["noisy"].shape[1] - L) for k in range(B)]
        noisy = np.stack([ex["noisy"][k % 5, s:s + L] for k, s in enumerate(starts)]).astype(np.float32) / 32768.0
        x = torch.from_numpy(noisy).cuda()
        y = torch.empty((B, 256 * (L // 256)), device="cuda")
        enhance = lambda: eng.forward_wave(x, win, out=y)
        enhance()
        ref = x[:, :y.shape[1]].contiguous()              # enhanced against noisy, as the golden excerpts are
        rec = torch.empty((B, 4), device="cuda", dtype=torch.float64)
        row = {"enhance_forward_wave_ms": median_ms(enhance, a.iters),
               "score_all_ms": median_ms(lambda: sc.score(ref, y, out=rec), a.iters),
               "score_sdr_sisnr_ms": median_ms(lambda: sc.score(ref, y, what=("sdr", "sisnr"), out=rec), a.iters)}
        row["score_over_enhance"] = row["score_all_ms"][0] / row["enhance_forward_wave_ms"][0]
        row["sdr_sisnr_over_enhance"] = row["score_sdr_sisnr_ms"][0] / row["enhance_forward_wave_ms"][0]
        sc.timing(True)
        stages = {}
        for _ in range(50):
            sc.score(ref, y, out=rec)
            for name, ms in sc.timing_read().items():
                stages.setdefault(name, []).append(ms)
        sc.timing(False)
        med = {k: statistics.median(v) for k, v in stages.items()}
        tot = sum(med.values())
        row["launch_ms"] = med
        row["launch_share"] = {k: v / tot for k, v in med.items()}
        row["mean_stoi"] = float(rec[:, 2].mean())
        res["batches"][f"B{B}"] = row
        print(f"B={B}: enhance {row['enhance_forward_wave_ms'][0]:.4f} ms, score {row['score_all_ms'][0]:.4f} ms "
              f"(x{row['score_over_enhance']:.2f}), SDR+SI-SNR {row['score_sdr_sisnr_ms'][0]:.4f} ms; launches "
              + ", ".join(f"{k} {v * 1e3:.1f} us" for k, v in med.items()), flush=True)
    # CPU context: our float64 checker, per clip, single process
    pairs = [SC.excerpt_pair(ex, c, o, L) for c, o in SC.EXCERPTS[:6]]
    SC.score(*pairs[0])
    t = time.perf_counter()
    for r, yy in pairs:
        SC.score(r, yy)
    res["cpu_float64_checker_s_per_clip"] = (time.perf_counter() - t) / len(pairs)
    res["cpu_note"] = "tests/score_checker.py (numpy / scipy, float64) on this host's CPU; our checker, not pystoi"
    print(f"float64 checker on the CPU: {res['cpu_float64_checker_s_per_clip'] * 1e3:.1f} ms per clip")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
