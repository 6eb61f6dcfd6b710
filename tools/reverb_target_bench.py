#!/usr/bin/env python3
"""What a dereverberation target costs next to the draw it extends and the train step it feeds (not a gate; bench.py is
untouched).

For B = 512 and B = 8 rows of 4 s (L = 64000), banks of 4096-tap and of 16384-tap responses, p_reverb = 0.5 and 1 and a
target of the direct path plus 50 ms, from tools/reverb_bench.py's corpus and banks, by its method (one process, warmed,
medians of device-event windows, every call draws new plans first), in the same run:
  (i)   today's draw: plans, gtcrn_batch_reverb, gtcrn_batch_mix -- clean is the full reverberant speech (unchanged code),
  (ii)  the composition the entry points of before allow for an early target: plans, gtcrn_batch_reverb on the bank,
        gtcrn_batch_reverb on a bank of the truncated responses into a second staged corpus, gtcrn_batch_mix, and the clean
        rows rewritten by torch from the second corpus (an int16 -> float copy and one multiply by Gf * 2^-15 per row),
  (iii) the fused draw: plans, gtcrn_batch_reverb_split, gtcrn_batch_mix_target,
  (iv)  the bf16_grads and the fp32 train step on a drawn batch,
each of (i) .. (iii) three times over, and the ratios (iii) / (ii), (iii) / (i), (iii) / step with the spread of the three
repetitions.  --rerun-reverb-bench also runs tools/reverb_bench.py in this process and puts its figures beside the committed
profiles/reverb_bench.json.

    python tools/reverb_target_bench.py [--out profiles/reverb_target_bench.json] [--iters 30] [--rerun-reverb-bench]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reverb_target_bench.json"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--train-iters", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gigabytes", type=float, default=2.0, help="least size of each side of the corpus")
    ap.add_argument("--batches", default="512,8")
    ap.add_argument("--taps", default="4096,16384")
    ap.add_argument("--p", default="0.5,1.0")
    ap.add_argument("--target-ms", type=float, default=50.0)
    ap.add_argument("--responses", type=int, default=64)
    ap.add_argument("--samples", type=int, default=64000)
    ap.add_argument("--rerun-reverb-bench", action="store_true")
    a = ap.parse_args(argv)
    import torch
    from batch_bench import median_ms, synthetic_corpus
    from reverb_bench import synthetic_bank
    from gtcrn_micro_amd._lib import _check, _stream_ptr, lib
    from gtcrn_micro_amd.data import BatchSource, RirBank
    from gtcrn_micro_amd.train import make_training, train_step
    assert torch.cuda.is_available(), "reverb_target_bench needs the GPU"
    L = a.samples
    nsamp = int(a.gigabytes * 1e9 / 2)
    speech, noise = synthetic_corpus(nsamp, 1), synthetic_corpus(nsamp, 2)
    banks = {K: synthetic_bank(a.responses, K, 3) for K in (int(v) for v in a.taps.split(","))}
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "L": L, "target_ms": a.target_ms,
           "corpus": {"speech_bytes": 2 * speech.pcm.numel(), "noise_bytes": 2 * noise.pcm.numel(), "clip_seconds": [5, 12]},
           "timing": "median (min, max) in ms over %d windows of 4 calls (train step: %d windows of 1), device events, warmed, one "
                     "process; (i) .. (iii) %d times over, `spread` = (largest - smallest median) / middle median"
                     % (a.iters, a.train_iters, a.reps),
           "batches": {}}
    for B in (int(v) for v in a.batches.split(",")):
        dry = BatchSource(speech, noise=noise, B=B, L=L, seed=1)
        row = {}
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
            split = bank.split_for(a.target_ms)
            taps, off = bank.taps.cpu().numpy(), bank.offsets.cpu().numpy()
            cut = RirBank.from_arrays([taps[int(off[r]):int(off[r]) + int(split[r])] for r in range(bank.n)], trim_direct=False)
            for p in (float(v) for v in a.p.split(",")):
                full = BatchSource(speech, noise=noise, B=B, L=L, seed=1, rirs=bank, p_reverb=p)
                fused = BatchSource(speech, noise=noise, B=B, L=L, seed=1, rirs=bank, p_reverb=p, target_ms=a.target_ms)
                comp = BatchSource(speech, noise=noise, B=B, L=L, seed=1, rirs=bank, p_reverb=p)
                stride = comp.staged_stride
                staged2 = torch.zeros_like(comp.staged)
                so2, sp2, rec2 = torch.zeros_like(comp.staged_offsets), torch.zeros_like(comp.staged_plan), torch.zeros_like(comp.reverb_records)
                scale = torch.zeros((B, 1), device="cuda")

                def reverb(bk, staged, so, splan, rec):
                    _check(lib().gtcrn_batch_reverb(
                        speech.pcm.data_ptr(), speech.offsets.data_ptr(), speech.n, bk.taps.data_ptr(), bk.offsets.data_ptr(), bk.n,
                        bk.table.data_ptr(), bk.table.numel(), comp.plan.data_ptr(), comp.reverb_plan.data_ptr(), B, L,
                        staged.data_ptr(), stride, so.data_ptr(), splan.data_ptr(), rec.data_ptr(), comp._rws.data_ptr(), 0,
                        _stream_ptr()))

                def composition():
                    comp.draw_reverb_plan()
                    comp.draw_plan()
                    reverb(bank, comp.staged, comp.staged_offsets, comp.staged_plan, comp.reverb_records)
                    reverb(cut, staged2, so2, sp2, rec2)
                    _check(lib().gtcrn_batch_mix(comp.staged.data_ptr(), comp.staged_offsets.data_ptr(), B, noise.pcm.data_ptr(),
                                                 noise.offsets.data_ptr(), noise.n, comp.staged_plan.data_ptr(), B, L,
                                                 comp.noisy.data_ptr(), L, comp.clean.data_ptr(), L, comp.records.data_ptr(),
                                                 comp._ws.data_ptr(), 7, _stream_ptr()))
                    torch.mul(comp.records[:, 7:8].view(torch.float32), 2.0 ** -15, out=scale)
                    comp.clean.copy_(staged2.view(B, stride)[:, :L])
                    comp.clean.mul_(scale)

                reps = []
                for _ in range(a.reps):
                    reps.append({"full_draw_ms": median_ms(lambda: full.draw(), a.iters),
                                 "composition_ms": median_ms(composition, a.iters),
                                 "fused_draw_ms": median_ms(lambda: fused.draw(), a.iters)})
                # the composition computes what the fused draw computes (the float pass rounds once more, so up to an ulp)
                fused.set_step(7)
                comp.set_step(7)
                fn, fc = fused.draw()
                composition()
                torch.cuda.synchronize()
                same_noisy = bool(torch.equal(fn, comp.noisy))
                clean_err = float((fc - comp.clean).abs().max() / fc.abs().max().clamp_min(1e-30))
                r = {"repetitions": reps, "composition_noisy_equals_fused": same_noisy, "composition_clean_rel_err": clean_err}
                for k in ("full_draw_ms", "composition_ms", "fused_draw_ms"):
                    med = sorted(x[k][0] for x in reps)
                    r[k] = med[len(med) // 2]
                    r[k.replace("_ms", "_spread")] = (med[-1] - med[0]) / med[len(med) // 2]
                r["fused_over_composition"] = r["fused_draw_ms"] / r["composition_ms"]
                r["fused_over_full"] = r["fused_draw_ms"] / r["full_draw_ms"]
                r["fused_over_train_step_f32"] = r["fused_draw_ms"] / row["train_step_f32_ms"][0]
                r["fused_over_train_step_bf16_grads"] = r["fused_draw_ms"] / row["train_step_bf16_grads_ms"][0]
                r["split_taps"] = [int(split.min()), int(split.max())]
                rec = fused.split_records_numpy()
                r["last_draw"] = {"wet_rows": int((rec["rir"] >= 0).sum()), "saturated_samples": int(rec["saturated"].sum()),
                                  "target_saturated_samples": int(rec["target_saturated"].sum())}
                row.setdefault(f"K{K}", {})[f"p{p:g}"] = r
                print(f"B={B} K={K} p={p:g}: full draw {r['full_draw_ms']:.3f} ms, composition {r['composition_ms']:.3f} ms, fused "
                      f"{r['fused_draw_ms']:.3f} ms (spreads {r['full_draw_spread']:.3f} / {r['composition_spread']:.3f} / "
                      f"{r['fused_draw_spread']:.3f}); fused / composition {r['fused_over_composition']:.3f}, fused / full "
                      f"{r['fused_over_full']:.3f}, fused / bf16_grads step {r['fused_over_train_step_bf16_grads']:.4f}; noisy equal "
                      f"{same_noisy}, clean rel err {clean_err:.2e}", flush=True)
                del full, fused, comp, staged2
                torch.cuda.empty_cache()
            del cut
        res["batches"][f"B{B}"] = row
    if a.rerun_reverb_bench:
        import reverb_bench
        del speech, noise, banks
        torch.cuda.empty_cache()
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "reverb_bench.json")
            reverb_bench.main(["--out", out, "--iters", str(a.iters)])
            now = json.load(open(out))
        then = json.load(open(os.path.join(ROOT, "profiles", "reverb_bench.json")))
        beside = {}
        for B, brow in now["batches"].items():
            for K in (k for k in brow if k.startswith("K")):
                for p, x in brow[K].items():
                    y = then["batches"].get(B, {}).get(K, {}).get(p)
                    beside[f"{B} {K} {p}"] = {f: {"now": x[f] if not isinstance(x[f], list) else x[f][0],
                                                  "committed": None if y is None else (y[f] if not isinstance(y[f], list) else y[f][0])}
                                              for f in ("matrix_ms", "matrix_2048_ms", "matrix_8192_ms", "draw_ms")}
        res["reverb_bench_rerun"] = beside
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
