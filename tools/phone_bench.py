#!/usr/bin/env python3
"""What telephone-channel rows cost next to the draw they follow and the train step they feed (not a gate; bench.py is
untouched).

For B = 512 rows of 4 s (L = 64000), from a synthetic corpus (tools/batch_bench.synthetic_corpus), in one process: warmed
medians over device events of
  * the mix draw with p_phone = 0 (the source without the channel), p_phone = 1 (every codec) and p_phone = 0.5,
  * the channel launch alone (gtcrn_batch_phone on the raw rows of the last draw) under the p_phone = 1 and 0.5 plans,
  * a float copy of the same rows (noisy and clean: 8 B read + 8 B written per sample and row),
  * a bf16_grads train step on a drawn batch.
The forms are taken in turn, `--reps` times over (alternating, so that a drift of the machine lands on every form alike); the
figures quoted are the medians over the repetitions of each repetition's median, with the spread between repetitions beside
them.  Derived: the channel's share of the train step, its ratio to the copy, and the v_dot2_i32_i16 rate it reaches, counted
from the kernel's geometry (130 per pair of 8 kHz samples and 130 per four outputs, halo included), against the vector
issue rate of gfx950 (one wave64 VALU instruction per SIMD every 2 cycles at 2.4 GHz with several waves resident).

    python tools/phone_bench.py [--out profiles/phone_bench.json] [--iters 40] [--reps 5] [--gigabytes 1.0]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CLOCK_HZ, CUS, SIMDS, VALU_CYCLES = 2.4e9, 256, 4, 2.0      # the issue-rate bound the dot2 rate is read against


def span(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phone_bench.json"))
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--train-iters", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gigabytes", type=float, default=1.0, help="least size of each side of the corpus")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--samples", type=int, default=64000)
    a = ap.parse_args(argv)
    import torch
    from batch_bench import median_ms, synthetic_corpus
    from gtcrn_micro_amd._lib import _check, _stream_ptr, lib
    from gtcrn_micro_amd.data import PHONE_TARGETS, BatchSource, phone_chunk
    from gtcrn_micro_amd.train import make_training, train_step
    assert torch.cuda.is_available(), "phone_bench needs the GPU"
    B, L = a.batch, a.samples
    nsamp = int(a.gigabytes * 1e9 / 2)
    speech, noise = synthetic_corpus(nsamp, 1), synthetic_corpus(nsamp, 2)
    src = {"p0": BatchSource(speech, noise=noise, B=B, L=L, seed=1),
           "p1": BatchSource(speech, noise=noise, B=B, L=L, seed=1, p_phone=1.0),
           "p05": BatchSource(speech, noise=noise, B=B, L=L, seed=1, p_phone=0.5)}

    def channel(s):
        def run():
            _check(lib().gtcrn_batch_phone(s._raw_noisy.data_ptr(), s._raw_noisy.stride(0), s._raw_clean.data_ptr(),
                                           s._raw_clean.stride(0), s.phone_plan.data_ptr(), B, L, s.noisy.data_ptr(), L,
                                           s.clean.data_ptr(), L, PHONE_TARGETS[s.phone_target], s.phone_records.data_ptr(),
                                           _stream_ptr()))
        return run

    def copy():
        s = src["p1"]
        s.noisy.copy_(s._raw_noisy)
        s.clean.copy_(s._raw_clean)

    for s in src.values():
        s.draw()
    torch.manual_seed(43)
    model, opt, sched, loss_func = make_training(device="cuda")
    model.set_activation_storage("bf16_grads")
    model.train()
    noisy, clean = src["p05"].draw()
    noisy, clean = noisy.clone(), clean.clone()
    forms = {"draw_p0": (lambda: src["p0"].draw(), a.iters, 10, 4), "draw_p1": (lambda: src["p1"].draw(), a.iters, 10, 4),
             "draw_p05": (lambda: src["p05"].draw(), a.iters, 10, 4), "channel_p1": (channel(src["p1"]), a.iters, 10, 4),
             "channel_p05": (channel(src["p05"]), a.iters, 10, 4), "copy": (copy, a.iters, 10, 4),
             "train_step_bf16_grads": (lambda: train_step(model, opt, sched, loss_func, noisy, clean), a.train_iters, 3, 1)}
    reps = []
    for _ in range(a.reps):
        reps.append({k: median_ms(fn, it, warmup=w, per=per) for k, (fn, it, w, per) in forms.items()})
    ms = {k: span([r[k][0] for r in reps]) for k in forms}
    ratio = lambda x, y: span([r[x][0] / r[y][0] for r in reps])      # noqa: E731
    C = phone_chunk()
    chunks = (L + C - 1) // C
    dot2_per_chunk = 130 * (C // 4 + 33) + 130 * (C // 4)            # per workgroup: the w pairs (halo included), the fours of outputs
    counts = src["p1"].phone_plan_numpy()["codec"]
    dot2 = 2 * B * chunks * dot2_per_chunk                           # p_phone = 1, target narrow: both sides of every row
    t = ms["channel_p1"]["median"] * 1e-3
    peak = CUS * SIMDS * 64 / VALU_CYCLES * CLOCK_HZ
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "B": B, "L": L, "chunk": C,
           "corpus": {"speech_bytes": 2 * speech.pcm.numel(), "noise_bytes": 2 * noise.pcm.numel()},
           "timing": "per repetition: median (min, max) in ms over %d windows of 4 calls (train step: %d windows of 1), device "
                     "events, warmed; %d repetitions, the forms in turn; the summary is the span of the repetitions' medians"
                     % (a.iters, a.train_iters, a.reps),
           "reps": reps, "ms": ms,
           "p1_codecs": {str(c): int((counts == c).sum()) for c in (-1, 0, 1, 2)},
           "p05_phone_rows": int((src["p05"].phone_plan_numpy()["codec"] >= 0).sum()),
           "channel_p1_over_train_step": ratio("channel_p1", "train_step_bf16_grads"),
           "channel_p05_over_train_step": ratio("channel_p05", "train_step_bf16_grads"),
           "channel_p1_over_copy": ratio("channel_p1", "copy"), "channel_p05_over_copy": ratio("channel_p05", "copy"),
           "draw_p1_minus_p0_ms": span([r["draw_p1"][0] - r["draw_p0"][0] for r in reps]),
           "draw_p05_minus_p0_ms": span([r["draw_p05"][0] - r["draw_p0"][0] for r in reps]),
           "dot2": {"lane_ops": dot2, "multiply_adds": 2 * dot2, "per_output_sample": dot2 / (2.0 * B * L),
                    "lane_ops_per_s": dot2 / t, "bound_lane_ops_per_s": peak, "share_of_bound": dot2 / t / peak,
                    "bound": "%d CUs x %d SIMDs x 64 lanes every %.0f cycles at %.1f GHz" % (CUS, SIMDS, VALU_CYCLES, CLOCK_HZ / 1e9)},
           "bytes": {"channel": 16 * B * L, "bytes_per_s": 16 * B * L / t}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    m = lambda k: ms[k]["median"]      # noqa: E731
    print(f"B={B} L={L}: draw p=0 {m('draw_p0'):.4f} ms, p=1 {m('draw_p1'):.4f} ms, p=0.5 {m('draw_p05'):.4f} ms; channel alone "
          f"p=1 {m('channel_p1'):.4f} ms, p=0.5 {m('channel_p05'):.4f} ms; copy {m('copy'):.4f} ms; train step bf16_grads "
          f"{m('train_step_bf16_grads'):.3f} ms; channel / step {res['channel_p1_over_train_step']['median']:.4f}, channel / copy "
          f"{res['channel_p1_over_copy']['median']:.2f}; dot2 {dot2 / t / 1e12:.2f} T lane-ops/s = "
          f"{100 * res['dot2']['share_of_bound']:.1f} % of the issue bound", flush=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
