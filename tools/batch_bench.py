#!/usr/bin/env python3
"""What drawing a training batch from a resident corpus costs next to the train step it feeds (not a gate; bench.py is
untouched).

For B = 512 and B = 8 rows of 4 s (L = 64000), from a synthetic corpus of at least 2 GB per side (random clips of 5 to
12 s, so the windows of a batch cannot all sit in a cache): warmed medians, device events, one process, of
  * a mix draw (plan + the three passes), and draws cut short after the plan, the sums and the peak pass
    (gtcrn_batch_mix's `passes`), whose differences are each launch's time,
  * a pairs draw (plan + one pass),
  * the fp32 and bf16_grads train step on a drawn batch,
  * a plain device copy that moves the draw's compulsory bytes (4 B read + 8 B written per output sample: a copy of
    6 B per sample, its source walking through the corpus so that it is not served from a cache either),
and the two ratios draw / train step and draw / copy.

    python tools/batch_bench.py [--out profiles/batch_bench.json] [--iters 100] [--gigabytes 2.0]

--active measures only the draw at an SNR of active levels (BatchSource(active_db=-50), 100 ms windows) beside the plain mix
draw, from the same corpora in the same run: the whole draw and each pass of both, repeated `--reps` times, and the ratios
active / plain with their spread between repetitions (profiles/batch_active_bench.json).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, iters, warmup=10, per=4):
    """Median (min, max) over `iters` windows of `per` back-to-back calls each, timed with device events."""
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


def synthetic_corpus(samples, seed, device="cuda"):
    """At least `samples` int16 samples of uniform noise cut into clips of 5 .. 12 s at 16 kHz."""
    import torch
    from gtcrn_micro_amd.data import Corpus
    rng = np.random.default_rng(seed)
    lens = []
    while sum(lens) < samples:
        lens.append(int(rng.integers(5 * 16000, 12 * 16000 + 1)))
    total = sum(lens)
    g = torch.Generator(device=device).manual_seed(seed)
    pcm = torch.empty(total, device=device, dtype=torch.int16)
    piece = 1 << 27
    for lo in range(0, total, piece):
        n = min(piece, total - lo)
        pcm[lo:lo + n] = torch.randint(-8000, 8000, (n,), device=device, dtype=torch.int16, generator=g)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(device)
    return Corpus.from_tensors(pcm, off)


def mix_times(src, iters):
    """A mix source's whole draw and each launch's share, as main() takes them: from draws cut short after the plan, the sums
    and the peak pass, every one of which draws a new plan first."""
    draw = median_ms(lambda: src.draw(), iters)
    cum = {"plan": median_ms(lambda: src.draw_plan(), iters),
           "plan_sums": median_ms(lambda: src.draw(passes=1), iters),
           "plan_sums_peak": median_ms(lambda: src.draw(passes=3), iters)}
    return {"draw_ms": draw, "cumulative_ms": cum,
            "launch_ms": {"plan": cum["plan"][0], "sums": cum["plan_sums"][0] - cum["plan"][0],
                          "peak": cum["plan_sums_peak"][0] - cum["plan_sums"][0], "write": draw[0] - cum["plan_sums_peak"][0]}}


def active_leg(a, speech, noise, L, res):
    """--active: the draw at an SNR of active levels (100 ms windows, -50 dB) beside the plain mix draw of the same run, B = 512:
    `reps` repetitions of both, interleaved; the ratios active / plain of the draw and of pass 1 per repetition, and the spread
    between repetitions they are to be read against."""
    from gtcrn_micro_amd.data import BatchSource, achieved_snr_db
    B, W, db = a.active_batch, 1600, -50.0
    plain = BatchSource(speech, noise=noise, B=B, L=L, seed=1)
    act = BatchSource(speech, noise=noise, B=B, L=L, seed=1, active_db=db, active_window=W)
    reps = []
    for _ in range(a.reps):
        reps.append({"plain": mix_times(plain, a.iters), "active": mix_times(act, a.iters)})
    col = lambda side, f: [f(r[side]) for r in reps]      # noqa: E731
    span = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}      # noqa: E731
    summary = {}
    for side in ("plain", "active"):
        summary[side] = {"draw_ms": span(col(side, lambda t: t["draw_ms"][0]))}
        for k in ("plan", "sums", "peak", "write"):
            summary[side][k + "_ms"] = span(col(side, lambda t, k=k: t["launch_ms"][k]))
    ratio = lambda f: span([f(r["active"]) / f(r["plain"]) for r in reps])      # noqa: E731
    summary["active_over_plain"] = {"draw": ratio(lambda t: t["draw_ms"][0])}
    for k in ("sums", "peak", "write"):
        summary["active_over_plain"][k] = ratio(lambda t, k=k: t["launch_ms"][k])
    act.draw()                                           # a whole draw last: the records below belong to the plan below
    rec = act.records_numpy()
    snr_active, snr_plain = achieved_snr_db(rec)
    res.update({"B": B, "window": W, "active_db": db, "threshold": act.active_threshold, "reps": reps, "summary": summary,
                "bytes_compulsory": 12 * B * L,
                "last_batch": {"flags_seen": sorted(set(int(v) for v in rec["flags"])),
                               "speech_active_share": float((rec["Ns"] / L).mean()), "noise_active_share": float((rec["Nn"] / L).mean()),
                               "snr_error_db_max": float(np.nanmax(np.abs(snr_active - act.plan_numpy()["snr_db"]))),
                               "plain_minus_active_snr_db_max": float(np.nanmax(np.abs(snr_plain - snr_active)))}})
    s = summary
    print(f"B={B} W={W} {db} dB: active draw {s['active']['draw_ms']['median']:.4f} ms (sums {s['active']['sums_ms']['median']:.4f}, "
          f"peak {s['active']['peak_ms']['median']:.4f}, write {s['active']['write_ms']['median']:.4f}); plain draw "
          f"{s['plain']['draw_ms']['median']:.4f} ms (sums {s['plain']['sums_ms']['median']:.4f}, peak "
          f"{s['plain']['peak_ms']['median']:.4f}, write {s['plain']['write_ms']['median']:.4f}); active / plain: draw "
          f"{s['active_over_plain']['draw']['median']:.3f}, sums {s['active_over_plain']['sums']['median']:.3f}", flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--active", action="store_true", help="only the active-level leg (default --out: profiles/batch_active_bench.json)")
    ap.add_argument("--active-batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5, help="repetitions of the active leg")
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--train-iters", type=int, default=12)
    ap.add_argument("--gigabytes", type=float, default=2.0, help="least size of each side of the corpus")
    ap.add_argument("--batches", default="512,8")
    ap.add_argument("--samples", type=int, default=64000)
    a = ap.parse_args(argv)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "batch_active_bench.json" if a.active else "batch_bench.json")
    import torch
    from gtcrn_micro_amd.data import BatchSource, Corpus
    from gtcrn_micro_amd.train import make_training, train_step
    assert torch.cuda.is_available(), "batch_bench needs the GPU"
    L = a.samples
    nsamp = int(a.gigabytes * 1e9 / 2)
    speech, noise = synthetic_corpus(nsamp, 1), synthetic_corpus(nsamp, 2)
    # the pairs form wants two buffers under ONE offsets table: the noise side's samples, cut like the speech side
    m = min(speech.pcm.numel(), noise.pcm.numel())
    keep = int((speech.offsets <= m).sum()) - 1
    paired_noisy = Corpus.from_tensors(speech.pcm, speech.offsets[:keep + 1].contiguous())
    paired_clean = Corpus.from_tensors(noise.pcm, speech.offsets[:keep + 1].contiguous())
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "L": L,
           "corpus": {"speech_bytes": 2 * speech.pcm.numel(), "speech_clips": speech.n, "noise_bytes": 2 * noise.pcm.numel(),
                      "noise_clips": noise.n, "clip_seconds": [5, 12]},
           "timing": "median (min, max) in ms over %d windows of 4 calls (train step: %d windows of 1), device events, warmed, "
                     "one process" % (a.iters, a.train_iters),
           "batches": {}}
    if a.active:
        del res["batches"]
        res["timing"] = "median (min, max) in ms over %d windows of 4 calls, device events, warmed, one process" % a.iters
        active_leg(a, speech, noise, L, res)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
        print("wrote", a.out)
        return
    for B in (int(v) for v in a.batches.split(",")):
        mix = BatchSource(speech, noise=noise, B=B, L=L, seed=1)
        prs = BatchSource(paired_noisy, paired_clean=paired_clean, B=B, L=L, seed=1)
        row = {"mix_draw_ms": median_ms(lambda: mix.draw(), a.iters), "pairs_draw_ms": median_ms(lambda: prs.draw(), a.iters)}
        # each launch's share, from draws cut short after the plan, the sums and the peak pass: every one of them draws a
        # new plan first, so the windows are as cold (or as warm) as in a full draw
        cum = {"plan": median_ms(lambda: mix.draw_plan(), a.iters),
               "plan_sums": median_ms(lambda: mix.draw(passes=1), a.iters),
               "plan_sums_peak": median_ms(lambda: mix.draw(passes=3), a.iters)}
        row["mix_cumulative_ms"] = cum
        row["mix_launch_ms"] = {"plan": cum["plan"][0], "sums": cum["plan_sums"][0] - cum["plan"][0],
                                "peak": cum["plan_sums_peak"][0] - cum["plan_sums"][0],
                                "write": row["mix_draw_ms"][0] - cum["plan_sums_peak"][0]}
        # the compulsory bytes as a plain copy: 6 B per output sample, read once and written once = 12 B moved
        nbytes = 6 * B * L
        src8 = speech.pcm.view(torch.uint8)
        dst = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
        span = src8.numel() - nbytes
        state = {"k": 0}

        def copy():
            lo = (state["k"] * 268435459) % span // 16 * 16
            state["k"] += 1
            dst.copy_(src8[lo:lo + nbytes])
        row["copy_ms"] = median_ms(copy, a.iters)
        row["copy_bytes_moved"] = 2 * nbytes
        row["draw_bytes_compulsory"] = 12 * B * L
        noisy, clean = mix.draw()
        for storage in ("f32", "bf16_grads"):
            torch.manual_seed(43)
            model, opt, sched, loss_func = make_training(device="cuda")
            if storage != "f32":
                model.set_activation_storage(storage)
            model.train()
            row[f"train_step_{storage}_ms"] = median_ms(lambda: train_step(model, opt, sched, loss_func, noisy, clean),
                                                        a.train_iters, warmup=3, per=1)
            del model, opt, sched, loss_func
        row["mix_over_train_step_f32"] = row["mix_draw_ms"][0] / row["train_step_f32_ms"][0]
        row["mix_over_train_step_bf16_grads"] = row["mix_draw_ms"][0] / row["train_step_bf16_grads_ms"][0]
        row["pairs_over_train_step_bf16_grads"] = row["pairs_draw_ms"][0] / row["train_step_bf16_grads_ms"][0]
        row["mix_over_copy"] = row["mix_draw_ms"][0] / row["copy_ms"][0]
        row["pairs_over_copy"] = row["pairs_draw_ms"][0] / row["copy_ms"][0]
        row["mix_flags_seen"] = sorted(set(int(v) for v in mix.records_numpy()["flags"]))
        res["batches"][f"B{B}"] = row
        print(f"B={B}: mix {row['mix_draw_ms'][0]:.4f} ms (plan {row['mix_launch_ms']['plan']:.4f}, sums "
              f"{row['mix_launch_ms']['sums']:.4f}, peak {row['mix_launch_ms']['peak']:.4f}, write "
              f"{row['mix_launch_ms']['write']:.4f}), pairs {row['pairs_draw_ms'][0]:.4f} ms, copy {row['copy_ms'][0]:.4f} ms, "
              f"train step fp32 {row['train_step_f32_ms'][0]:.3f} / bf16_grads {row['train_step_bf16_grads_ms'][0]:.3f} ms; "
              f"mix / step {row['mix_over_train_step_bf16_grads']:.4f}, mix / copy {row['mix_over_copy']:.2f}, "
              f"pairs / copy {row['pairs_over_copy']:.2f}", flush=True)
        del mix, prs, dst, noisy, clean
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
