#!/usr/bin/env python3
"""What the tone guard costs next to the plain step (not a gate; bench.py is untouched).

Shapes: the hop form (one 256-sample hop per call) and the packet form at 16 kHz / 160 (a window is one period: 8 calls,
5 hops), each at 16 384 and 65 536 resident streams.  Forms, on ONE state per shape so all three touch the same memory:
  plain   the state without tones (k_wave_synthesis)
  detect  tones="detect": the records advance, the output is the plain one (the Guard instantiation, mode 0)
  guard   tones=True: the defaults, blocks that hold a tone are passed dry
Each form is warmed; three alternating repetitions (plain, detect, guard, plain, ...) in one process; per form the median over
the repetitions of each repetition's median window, device events.  The spread is (max - min) / median of a form's three
repetitions: a ratio inside it is not a difference.  The yardstick is the plain step of the same run.
A second pass of three repetitions times the synthesis launch alone, from the library's launch records (an event pair
around k_wave_synthesis alone, the row a launch with tones and no gains or meters is timed in).

    python tools/tone_bench.py [--out profiles/tone_bench.json] [--iters 30]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ("plain", "detect", "guard")
ROW = {f: "k_wave_synthesis" for f in FORMS}      # a launch with tones is timed in the row of the form it stands in for


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


def measure(eng, step, st, iters, per):
    """step(i): one call of the shape.  Returns {form: [median window of each repetition]} and, from the launch records of
    a pass of its own, {form: [the synthesis launch's mean ms]}."""
    import torch
    from gtcrn_micro_amd import tone_params, tone_table
    records = torch.zeros((st.n, 8), device="cuda")
    table = torch.from_numpy(tone_table()).cuda()
    words = {"detect": torch.from_numpy(tone_params(mode=0)).cuda(), "guard": torch.from_numpy(tone_params()).cuda()}

    def select(form):
        st.tones = None if form == "plain" else records
        st.tone_params = None if form == "plain" else words[form]
        st.tone_table = None if form == "plain" else table
        if form != "plain":
            st.reset_tones()

    reps = {f: [] for f in FORMS}
    for _ in range(3):
        for form in FORMS:
            select(form)
            reps[form].append(statistics.median(windows_ms(step, iters, 3, per)))
    kern = {f: [] for f in FORMS}
    for _ in range(3):
        for form in FORMS:
            select(form)
            for i in range(3 * per):
                step(i % per)
            eng.timing_enable(True, only=ROW[form])
            for i in range(20 * per):
                step(i % per)
            torch.cuda.synchronize()
            kern[form].append(eng.timing_read()[ROW[form]][0])
            eng.timing_enable(False)
    select("plain")
    return reps, kern


def tone_block_of(n):
    """n samples of the digit 5 (770 + 1336 Hz), amplitude 0.1 per tone.  The same samples are fed at every call, so the phase
    jumps between blocks; inside a block the pair is pure, which is all the detector looks at."""
    import torch
    t = torch.arange(n, device="cuda") / 16000.0
    return 0.1 * (torch.sin(2 * np.pi * 770 * t) + torch.sin(2 * np.pi * 1336 * t))


def summary(measured):
    reps, kern = measured
    med = {f: statistics.median(v) for f, v in reps.items()}
    row = {f + "_ms": med[f] for f in FORMS}
    row["repetitions_ms"] = reps
    row["spread"] = {f: (max(v) - min(v)) / med[f] for f, v in reps.items()}
    row["detect_over_plain"] = med["detect"] / med["plain"]
    row["guard_over_plain"] = med["guard"] / med["plain"]
    kmed = {f: statistics.median(v) for f, v in kern.items()}
    row["synthesis_kernel_ms"] = kmed
    row["synthesis_kernel_repetitions_ms"] = kern
    row["synthesis_kernel_spread"] = {f: (max(v) - min(v)) / kmed[f] for f, v in kern.items()}
    return row


def report(name, row):
    print("%s: plain %.4f ms per call, detect x%.4f, guard x%.4f (spreads %s)" % (
        name, row["plain_ms"], row["detect_over_plain"], row["guard_over_plain"],
        ", ".join("%s %.4f" % kv for kv in row["spread"].items())), flush=True)
    print("  synthesis launch: " + ", ".join("%s %.2f us" % (f, 1e3 * v) for f, v in row["synthesis_kernel_ms"].items()),
          flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tone_bench.json"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--streams", type=int, nargs="*", default=[16384, 65536])
    ap.add_argument("--packet-streams", type=int, nargs="*", default=[16384, 65536])
    a = ap.parse_args(argv)
    import torch
    from gtcrn_micro_amd import Engine, make_window
    assert torch.cuda.is_available(), "tone_bench needs the GPU"
    params = np.fromfile(os.path.join(ROOT, "tests", "golden", "params_dns3.f32"), dtype=np.float32)
    eng = Engine(params, 0)
    win = torch.from_numpy(make_window(0)).cuda()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "timing": "per call; median over 3 alternating repetitions of the median of %d windows, device events, 3 warm-up "
                     "windows per repetition" % a.iters,
           "spread": "(max - min) / median of a form's three repetitions", "shapes": {}}
    gen = torch.Generator(device="cuda").manual_seed(1)
    for n in a.streams:
        st = eng.new_wave_state(n, win)
        x = torch.randn(n, 256, device="cuda", generator=gen) * 0.1
        x[::4] = tone_block_of(256)                                # every fourth stream holds a digit: its blocks are guarded
        y = torch.empty_like(x)
        eng.reserve(n, 1)
        row = summary(measure(eng, lambda i: eng.wave_stream_step(st, x, out=y), st, a.iters, 10))
        row["window_calls"] = 10
        res["shapes"]["hop_form_%d_streams" % n] = row
        report("hop form, %d streams" % n, row)
        del st, x, y
        torch.cuda.empty_cache()
    for n in a.packet_streams:
        st = eng.new_packet_state(n, win, 160, 16000)
        x = torch.randn(n, 160, device="cuda", generator=gen) * 0.1
        x[::4] = tone_block_of(160)
        y = torch.empty_like(x)
        row = summary(measure(eng, lambda i: eng.packet_stream_step(st, x, out=y), st, a.iters, st.period))
        row["window_calls"] = st.period
        res["shapes"]["packet_form_16k_160_%d_streams" % n] = row
        report("packet form 16 kHz / 160, %d streams" % n, row)
        del st, x, y
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
