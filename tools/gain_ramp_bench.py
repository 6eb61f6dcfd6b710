#!/usr/bin/env python3
"""What the gain ramps cost next to the limited step they stand in for (not a gate; bench.py is untouched).

Shapes: the hop form (one 256-sample hop per call) at 16 384 and 65 536 resident streams, and the packet form at
16 kHz / 160 (a window is one period: 8 calls, 5 hops).  Forms, on ONE state per shape so all three touch the same memory:
  limited   the state without ramp words (k_wave_synthesis<MIX>)
  steady    ramp words set and p == g everywhere (the RAMP instantiation, its `p != g` branch not taken)
  ramping   every stream ramps in every wave step: the gains alternate between two arrays from one wave step to the next,
            so the word a step leaves is never the next one's gain.  The limited form alternates the same arrays; the
            steady form uses ONE array, which its words equal from the start of each repetition.
Each form is warmed; three alternating repetitions (limited, steady, ramping, limited, ...) in one process; per form the
median over the repetitions of each repetition's median window, device events.  The spread is (max - min) / median of a
form's three repetitions: a ratio inside it is not a difference.
A second pass of three repetitions times the one launch the ramp lives in, from the library's launch records (an event pair
around k_wave_synthesis_mix alone, the row a ramped launch is timed in): where a call's ratio leaves the spread, it says
how much of the call that launch is and by how much it moved.

    python tools/gain_ramp_bench.py [--out profiles/gain_ramp_bench.json] [--iters 30]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ("limited", "steady", "ramping")


def windows_ms(fn, iters, warmup, per):
    """Per-call times of `iters` windows of `per` back-to-back calls each, device events, after `warmup` windows."""
    import torch
    for _ in range(warmup):
        for i in range(per):
            fn(i)
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(per):
            fn(i)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / per)
    return out


def measure(eng, step, will_step, st, iters, per):
    """step(i): one call of the shape; will_step(): whether the next call runs the wave step (a packet call without a hop
    does not, and must not use up a gain change).  Returns {form: [median window of each repetition]} and, from the launch
    records of a pass of its own (an event pair around k_wave_synthesis_mix alone), {form: [that kernel's mean ms]}."""
    import torch
    ga = torch.full((st.n,), 0.5, device="cuda")
    gb = torch.full((st.n,), 0.25, device="cuda")
    words = torch.empty((st.n,), device="cuda")

    def call(form):
        odd = [False]

        def fn(i):
            # ramping: the word the last wave step left is the other array's gain; steady: one array, the word equals it
            if form != "steady" and will_step():
                odd[0] = not odd[0]
            st.set_dry_gain(gb if odd[0] else ga)
            step(i)
        return fn

    reps = {f: [] for f in FORMS}
    for _ in range(3):
        for form in FORMS:
            st.gain_ramp = None if form == "limited" else words
            words.copy_(ga)
            reps[form].append(statistics.median(windows_ms(call(form), iters, 3, per)))
    kern = {f: [] for f in FORMS}
    for _ in range(3):
        for form in FORMS:
            st.gain_ramp = None if form == "limited" else words
            words.copy_(ga)
            fn = call(form)
            for i in range(3 * per):
                fn(i % per)
            eng.timing_enable(True, only="k_wave_synthesis_mix")
            for i in range(20 * per):
                fn(i % per)
            torch.cuda.synchronize()
            kern[form].append(eng.timing_read()["k_wave_synthesis_mix"][0])
            eng.timing_enable(False)
    st.gain_ramp = None
    return reps, kern


def summary(measured):
    reps, kern = measured
    med = {f: statistics.median(v) for f, v in reps.items()}
    row = {f + "_ms": med[f] for f in FORMS}
    row["repetitions_ms"] = reps
    row["spread"] = {f: (max(v) - min(v)) / med[f] for f, v in reps.items()}
    row["steady_over_limited"] = med["steady"] / med["limited"]
    row["ramping_over_limited"] = med["ramping"] / med["limited"]
    kmed = {f: statistics.median(v) for f, v in kern.items()}
    row["synthesis_kernel_ms"] = kmed                     # the launch the ramp lives in, from the launch records
    row["synthesis_kernel_repetitions_ms"] = kern
    row["synthesis_kernel_spread"] = {f: (max(v) - min(v)) / kmed[f] for f, v in kern.items()}
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gain_ramp_bench.json"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--streams", type=int, nargs="*", default=[16384, 65536])
    ap.add_argument("--packet-streams", type=int, default=16384)
    a = ap.parse_args(argv)
    import torch
    from gtcrn_micro_amd import Engine, make_window
    assert torch.cuda.is_available(), "gain_ramp_bench needs the GPU"
    params = np.fromfile(os.path.join(ROOT, "tests", "golden", "params_dns3.f32"), dtype=np.float32)
    eng = Engine(params, 0)
    win = torch.from_numpy(make_window(0)).cuda()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "timing": "per call; median over 3 alternating repetitions of the median of %d windows, device events, 3 warm-up "
                     "windows per repetition" % a.iters,
           "spread": "(max - min) / median of a form's three repetitions", "shapes": {}}
    gen = torch.Generator(device="cuda").manual_seed(1)
    for n in a.streams:
        st = eng.new_wave_state(n, win, atten_lim_db=6)
        x = torch.randn(n, 256, device="cuda", generator=gen) * 0.1
        y = torch.empty_like(x)
        eng.reserve(n, 1)
        row = summary(measure(eng, lambda i: eng.wave_stream_step(st, x, out=y), lambda: True, st, a.iters, 10))
        row["window_calls"] = 10
        res["shapes"]["hop_form_%d_streams" % n] = row
        print("hop form, %d streams: limited %.4f ms, steady x%.4f, ramping x%.4f (spreads %s)" % (
            n, row["limited_ms"], row["steady_over_limited"], row["ramping_over_limited"],
            ", ".join("%s %.4f" % kv for kv in row["spread"].items())), flush=True)
        print("  k_wave_synthesis_mix: " + ", ".join("%s %.2f us" % (f, 1e3 * v) for f, v in row["synthesis_kernel_ms"].items()),
              flush=True)
        del st, x, y
        torch.cuda.empty_cache()
    n = a.packet_streams
    st = eng.new_packet_state(n, win, 160, 16000, atten_lim_db=6)
    x = torch.randn(n, 160, device="cuda", generator=gen) * 0.1
    y = torch.empty_like(x)
    row = summary(measure(eng, lambda i: eng.packet_stream_step(st, x, out=y), lambda: st.next_hops > 0, st, a.iters, st.period))
    row["window_calls"] = st.period
    res["shapes"]["packet_form_16k_160_%d_streams" % n] = row
    print("packet form 16 kHz / 160, %d streams: limited %.4f ms per call, steady x%.4f, ramping x%.4f (spreads %s)" % (
        n, row["limited_ms"], row["steady_over_limited"], row["ramping_over_limited"],
        ", ".join("%s %.4f" % kv for kv in row["spread"].items())), flush=True)
    print("  k_wave_synthesis_mix: " + ", ".join("%s %.2f us" % (f, 1e3 * v) for f, v in row["synthesis_kernel_ms"].items()),
          flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
