#!/usr/bin/env python3
"""What the packet loss concealment costs next to a copy of its rows and the live step it precedes (not a gate; bench.py is
untouched).

65 536 streams in one process; four forms -- 16 kHz / 160 float32 and int16, 8 kHz / 160 mu-law, 48 kHz / 480 float32 -- each at
four loss patterns:
  * loss_0     no row is lost: every row is read once and n int16 go into its ring,
  * loss_5     in every call another 5 % of the rows begin an erasure (the lag search runs), the 5 % of the call before
               recover (the cross-fade), 90 % are received: the flags rotate over 20 patterns,
  * loss_100   every row is lost in every call: a running erasure, no search (after the warm-up the fade has reached zero),
  * begin_all  calls alternate between all rows lost and all rows received, so every second call runs the lag search in all
               65 536 rows and the others the cross-fade: the mean of one call of each (a worst case no network produces).
Warmed medians over device events of Concealer.conceal, of a plain device copy of the same row bytes, and of the packet-slot step
of the same slots (the same rate, packet and row type), which a gateway runs next.  The forms are taken in turn, `--reps` times
over (alternating, so that a drift of the machine lands on every form alike); the figures quoted are the medians over the
repetitions of each repetition's median, with the spread between repetitions beside them.  Derived per case: the call as a
multiple of the copy, as a share of the packet-slot step, and as a share of the tick (the n / fs s in which the next packets
arrive).

    python tools/plc_bench.py [--out profiles/plc_bench.json] [--iters 20] [--reps 5] [--streams 65536]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FORMS = (("f32_16k_160", 16000, 160, "f32"), ("pcm16_16k_160", 16000, 160, "pcm16"), ("ulaw_8k_160", 8000, 160, "ulaw"),
         ("f32_48k_480", 48000, 480, "f32"))


def span(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plc_bench.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--no-step", action="store_true", help="leave the packet-slot steps out")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from batch_bench import median_ms
    from gtcrn_micro_amd import Concealer, Engine, f32_to_g711
    assert torch.cuda.is_available(), "plc_bench needs the GPU"
    S = a.streams
    gen = torch.Generator(device="cuda").manual_seed(7)
    level = torch.tensor([0.3, 0.1, 0.03, 1e-3], device="cuda")[torch.randint(0, 4, (S,), device="cuda", generator=gen)]
    row = torch.arange(S, device="cuda", dtype=torch.int32)
    rotate = [((row + k) % 20 == 0).to(torch.int32) for k in range(20)]
    none, every = torch.zeros(S, device="cuda", dtype=torch.int32), torch.ones(S, device="cuda", dtype=torch.int32)
    forms, info, keep = {}, {}, []
    eng = None
    if not a.no_step:
        eng = Engine(np.fromfile(os.path.join(ROOT, "tests", "golden", "params_dns3.f32"), dtype=np.float32), 0)
        win = torch.hann_window(512).pow(0.5).cuda()
    for name, fs, n, kind in FORMS:
        xf = torch.randn(S, n, device="cuda", generator=gen) * level[:, None]
        if kind == "f32":
            x, dt, law = xf, torch.float32, None
        elif kind == "pcm16":
            x, dt, law = (xf * 32768).round().clamp(-32768, 32767).to(torch.int16), torch.int16, None
        else:
            x, dt, law = f32_to_g711(xf, "ulaw"), torch.uint8, "ulaw"
        y = torch.zeros_like(x)
        forms["copy_" + name] = (lambda x=x, y=y: y.copy_(x), a.iters, 10, 4)
        for pattern in ("loss_0", "loss_5", "loss_100", "begin_all"):
            c = Concealer(S, fs, n, 0, dt, g711=law)
            work = x.clone()
            c.conceal(work.copy_(x), none)                        # a history to search in
            flags = {"loss_0": [none], "loss_5": rotate, "loss_100": [every], "begin_all": [every, none]}[pattern]
            tick = [0]

            def call(c=c, work=work, flags=flags, tick=tick):
                c.conceal(work, flags[tick[0] % len(flags)])
                tick[0] += 1
            key = "plc_%s_%s" % (name, pattern)
            forms[key] = (call, a.iters, 20, 2 if pattern == "begin_all" else 4)
            info[key] = (c, "copy_" + name, "step_" + name, n / fs * 1e3)
            keep.append((work, x))
        if eng is not None:
            st = eng.new_packet_slot_state(S, win, n, fs, g711=law)
            ys = torch.zeros_like(x)
            forms["step_" + name] = (lambda st=st, x=x, ys=ys: eng.packet_stream_step_slots(st, row, x, out=ys), max(a.iters // 2, 4), 3, 1)
    reps = []
    for _ in range(a.reps):
        reps.append({k: median_ms(fn, it, warmup=w, per=per) for k, (fn, it, w, per) in forms.items()})
    ms = {k: span([r[k][0] for r in reps]) for k in forms}
    cases = {}
    for key, (c, copy, step, tick_ms) in info.items():
        ev = c.events().sum(0).tolist()
        d = {"erasures": ev[0], "lost_packets": ev[1], "ms": ms[key], "over_copy": span([r[key][0] / r[copy][0] for r in reps]),
             "share_of_tick": span([r[key][0] / tick_ms for r in reps])}
        if eng is not None:
            d["share_of_packet_slot_step"] = span([r[key][0] / r[step][0] for r in reps])
        cases[key] = d
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "streams": S,
           "timing": "per repetition: median (min, max) in ms over %d windows of 4 calls (begin_all: of 2, one call of each kind; "
                     "packet-slot step: %d windows of 1), device events, warmed; %d repetitions, the forms in turn; the summary is the "
                     "span of the repetitions' medians; the event counters are modulo 65536 per stream"
                     % (a.iters, max(a.iters // 2, 4), a.reps),
           "reps": reps, "ms": ms, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    for key, d in cases.items():
        print("%-34s %8.4f ms  = %6.2f x copy, %6.3f %% of the tick%s" % (
            key, d["ms"]["median"], d["over_copy"]["median"], 100 * d["share_of_tick"]["median"],
            "" if eng is None else ", %6.3f %% of the packet-slot step" % (100 * d["share_of_packet_slot_step"]["median"])), flush=True)
    for k in forms:
        if k.startswith(("copy_", "step_")):
            print("%-34s %8.4f ms" % (k, ms[k]["median"]))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
