#!/usr/bin/env python3
"""What reverberating a training batch costs next to the draw and the train step it feeds (not a gate; bench.py is
untouched).

For B = 512 and B = 8 rows of 4 s (L = 64000), banks of 4096-tap and of 16384-tap responses, p_reverb = 0.5 and 1, from
a synthetic corpus of at least 2 GB per side (tools/batch_bench.py's: the windows of a batch cannot all sit in a cache):
warmed medians, device events, one process, of
  * the two plans alone, and the two plans + gtcrn_batch_reverb in its plain and in its matrix form: the difference is
    the convolution's time (every call draws new plans first, so its windows are as cold as in a draw); the matrix form
    also with its block pinned to 2048 and to 8192 output samples,
  * the whole draw (plans, convolution in the form the library chooses, mix), and the draw of the same source without a
    bank,
  * the fp32 and bf16_grads train step on a drawn batch,
and the ratios matrix / plain, draw / train step, and the matrix form's rate against the int8 MFMA peak: an int16 x int16
multiply-add is four int8 digit products, counted over the K taps and L outputs of every reverberant row (not over the
padding of the 64-tap chunks or of the last block), against 2 x the 2.5 PFLOP/s BF16 peak = 2.5e15 int8 MAC/s.

    python tools/reverb_bench.py [--out profiles/reverb_bench.json] [--iters 30] [--gigabytes 2.0]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

INT8_PEAK_MACS = 2.5e15       # I8 MFMA = 2 x BF16 per clock; BF16 peak ~2.5 PFLOP/s dense = 1.25e15 MAC/s


def synthetic_bank(n, K, seed, device="cuda"):
    """n responses of K taps: a direct path and an exponentially decaying tail, peak-normalised."""
    from gtcrn_micro_amd.data import RirBank
    rng = np.random.default_rng(seed)
    hs = []
    for _ in range(n):
        h = rng.standard_normal(K) * np.exp(-np.arange(K) * (6.9 / K)) * 0.1       # -60 dB at the last tap
        h[0] = 1.0
        hs.append(h)
    return RirBank.from_arrays(hs, normalize="peak", trim_direct=True, device=device)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reverb_bench.json"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--plain-iters", type=int, default=3)
    ap.add_argument("--train-iters", type=int, default=12)
    ap.add_argument("--gigabytes", type=float, default=2.0, help="least size of each side of the corpus")
    ap.add_argument("--batches", default="512,8")
    ap.add_argument("--taps", default="4096,16384")
    ap.add_argument("--p", default="0.5,1.0")
    ap.add_argument("--responses", type=int, default=64)
    ap.add_argument("--samples", type=int, default=64000)
    a = ap.parse_args(argv)
    import torch
    from batch_bench import median_ms, synthetic_corpus
    from gtcrn_micro_amd._lib import _check, _stream_ptr, lib
    from gtcrn_micro_amd.data import BatchSource
    from gtcrn_micro_amd.train import make_training, train_step
    assert torch.cuda.is_available(), "reverb_bench needs the GPU"
    L = a.samples
    nsamp = int(a.gigabytes * 1e9 / 2)
    speech, noise = synthetic_corpus(nsamp, 1), synthetic_corpus(nsamp, 2)
    banks = {K: synthetic_bank(a.responses, K, 3) for K in (int(v) for v in a.taps.split(","))}
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "L": L,
           "corpus": {"speech_bytes": 2 * speech.pcm.numel(), "noise_bytes": 2 * noise.pcm.numel(), "clip_seconds": [5, 12]},
           "banks": {str(K): {"responses": b.n, "taps": K, "table_bytes": b.table.numel()} for K, b in banks.items()},
           "int8_mfma_peak_macs_per_s": INT8_PEAK_MACS,
           "timing": "median (min, max) in ms over %d windows of 4 calls (plain form: %d windows of 1; train step: %d windows of "
                     "1), device events, warmed, one process" % (a.iters, a.plain_iters, a.train_iters),
           "batches": {}}
    for B in (int(v) for v in a.batches.split(",")):
        dry = BatchSource(speech, noise=noise, B=B, L=L, seed=1)
        row = {"dry_draw_ms": median_ms(lambda: dry.draw(), a.iters)}
        noisy, clean = dry.draw()
        for storage in ("f32", "bf16_grads"):
            torch.manual_seed(43)
            model, opt, sched, loss_func = make_training(device="cuda")
            if storage != "f32":
                model.set_activation_storage(storage)
            model.train()
            row[f"train_step_{storage}_ms"] = median_ms(lambda: train_step(model, opt, sched, loss_func, noisy, clean),
                                                        a.train_iters, warmup=3, per=1)
            del model, opt, sched, loss_func
        del dry, noisy, clean
        for K, bank in banks.items():
            for p in (float(v) for v in a.p.split(",")):
                src = BatchSource(speech, noise=noise, B=B, L=L, seed=1, rirs=bank, p_reverb=p)

                def plans():
                    src.draw_reverb_plan()
                    src.draw_plan()

                def reverb(form):
                    plans()
                    _check(lib().gtcrn_batch_reverb(
                        speech.pcm.data_ptr(), speech.offsets.data_ptr(), speech.n, bank.taps.data_ptr(), bank.offsets.data_ptr(),
                        bank.n, bank.table.data_ptr(), bank.table.numel(), src.plan.data_ptr(), src.reverb_plan.data_ptr(), B, L,
                        src.staged.data_ptr(), src.staged_stride, src.staged_offsets.data_ptr(), src.staged_plan.data_ptr(),
                        src.reverb_records.data_ptr(), src._rws.data_ptr(), form, _stream_ptr()))
                r = {"plans_ms": median_ms(plans, a.iters),
                     "plans_matrix_ms": median_ms(lambda: reverb(2), a.iters),
                     "plans_plain_ms": median_ms(lambda: reverb(1), a.plain_iters, warmup=1, per=1),
                     "plans_matrix_2048_ms": median_ms(lambda: reverb(3), a.iters),
                     "plans_matrix_8192_ms": median_ms(lambda: reverb(4), a.iters),
                     "draw_ms": median_ms(lambda: src.draw(), a.iters)}
                r["matrix_ms"] = r["plans_matrix_ms"][0] - r["plans_ms"][0]
                r["plain_ms"] = r["plans_plain_ms"][0] - r["plans_ms"][0]
                r["matrix_2048_ms"] = r["plans_matrix_2048_ms"][0] - r["plans_ms"][0]     # the block pinned (forms 3 and 4)
                r["matrix_8192_ms"] = r["plans_matrix_8192_ms"][0] - r["plans_ms"][0]
                r["matrix_over_plain"] = r["matrix_ms"] / r["plain_ms"]
                r["draw_over_dry_draw"] = r["draw_ms"][0] / row["dry_draw_ms"][0]
                r["draw_over_train_step_f32"] = r["draw_ms"][0] / row["train_step_f32_ms"][0]
                r["draw_over_train_step_bf16_grads"] = r["draw_ms"][0] / row["train_step_bf16_grads_ms"][0]
                r["int8_macs_per_draw_expected"] = 4.0 * p * B * L * K
                r["matrix_int8_macs_per_s"] = r["int8_macs_per_draw_expected"] / (r["matrix_ms"] * 1e-3)
                r["matrix_fraction_of_int8_peak"] = r["matrix_int8_macs_per_s"] / INT8_PEAK_MACS
                rec = src.reverb_records_numpy()
                r["last_draw"] = {"wet_rows": int((rec["rir"] >= 0).sum()), "saturated_samples": int(rec["saturated"].sum())}
                row.setdefault(f"K{K}", {})[f"p{p:g}"] = r
                print(f"B={B} K={K} p={p:g}: reverb matrix {r['matrix_ms']:.3f} ms (2048: {r['matrix_2048_ms']:.3f}, 8192: "
                      f"{r['matrix_8192_ms']:.3f}), plain {r['plain_ms']:.3f} ms (matrix / plain "
                      f"{r['matrix_over_plain']:.4f}), draw {r['draw_ms'][0]:.3f} ms (dry {row['dry_draw_ms'][0]:.3f}), train step fp32 "
                      f"{row['train_step_f32_ms'][0]:.2f} / bf16_grads {row['train_step_bf16_grads_ms'][0]:.2f} ms; draw / step "
                      f"{r['draw_over_train_step_bf16_grads']:.4f}; {r['matrix_fraction_of_int8_peak']:.3f} of the int8 peak",
                      flush=True)
                del src
                torch.cuda.empty_cache()
        res["batches"][f"B{B}"] = row
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
