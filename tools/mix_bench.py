#!/usr/bin/env python3
"""What the conference mix costs next to a copy of its bytes and the live step it follows (not a gate; bench.py is untouched).

65 536 participants in one process, float32 and int16 blocks of n = 160 and n = 320 samples, in three room layouts -- rooms of
4, rooms of 32, 64 rooms of 1024 -- each participant sending noise at one of four fixed levels, so that after the warm-up
every room has its K = 3 talkers and no fades (the steady state of a call).  Warmed medians over device events of
  * gtcrn_mix_rooms / _pcm16 through Mixer.mix, one call over all rooms,
  * a plain device copy of the same blocks (the mix's input bytes read, its output bytes written),
  * the packet-slot step (16 kHz / 160, float32) of the same 65 536 participants, which a bridge runs before the mix.
The forms are taken in turn, `--reps` times over (alternating, so that a drift of the machine lands on every form alike); the
figures quoted are the medians over the repetitions of each repetition's median, with the spread between repetitions beside
them.  Derived per case: the mix as a multiple of the copy, as a share of the packet-slot step, and as a share of the tick (the
n / 16000 s in which the next blocks arrive).

    python tools/mix_bench.py [--out profiles/mix_bench.json] [--iters 20] [--reps 5] [--participants 65536]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LAYOUTS = {"rooms_of_4": 4, "rooms_of_32": 32, "rooms_of_1024": 1024}


def span(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_bench.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--participants", type=int, default=65536)
    ap.add_argument("--no-step", action="store_true", help="leave the packet-slot step out")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from batch_bench import median_ms
    from gtcrn_micro_amd import Engine, Mixer
    assert torch.cuda.is_available(), "mix_bench needs the GPU"
    P = a.participants
    gen = torch.Generator(device="cuda").manual_seed(5)
    level = torch.tensor([0.3, 0.1, 0.03, 1e-3], device="cuda")[torch.randint(0, 4, (P,), device="cuda", generator=gen)]
    forms, info = {}, {}
    for n in (160, 320):
        xf = torch.randn(P, n, device="cuda", generator=gen) * level[:, None]
        for dt, name in ((torch.float32, "f32"), (torch.int16, "pcm16")):
            x = xf if dt == torch.float32 else (xf * 32768).round().clamp(-32768, 32767).to(torch.int16)
            y = torch.zeros_like(x)
            forms["copy_%s_n%d" % (name, n)] = (lambda x=x, y=y: y.copy_(x), a.iters, 10, 4)
            for layout, size in LAYOUTS.items():
                rooms = [list(range(r, min(r + size, P))) for r in range(0, P, size)]
                m = Mixer(P, len(rooms), P, 0)
                m.set_rooms(rooms)
                out = torch.zeros_like(x)
                key = "mix_%s_n%d_%s" % (name, n, layout)
                forms[key] = (lambda m=m, x=x, out=out: m.mix(x, out=out), a.iters, 10, 4)
                info[key] = (m, len(rooms), "copy_%s_n%d" % (name, n), n)
    if not a.no_step:
        params = np.fromfile(os.path.join(ROOT, "tests", "golden", "params_dns3.f32"), dtype=np.float32)
        eng = Engine(params, 0)
        st = eng.new_packet_slot_state(P, torch.hann_window(512).pow(0.5).cuda(), 160, 16000, alc="vad")
        slots = torch.arange(P, device="cuda", dtype=torch.int32)
        xs, ys = torch.randn(P, 160, device="cuda", generator=gen) * level[:, None], torch.zeros(P, 160, device="cuda")
        forms["packet_slot_step_16k_160"] = (lambda: eng.packet_stream_step_slots(st, slots, xs, out=ys), max(a.iters // 2, 4), 4, 1)
    reps = []
    for _ in range(a.reps):
        reps.append({k: median_ms(fn, it, warmup=w, per=per) for k, (fn, it, w, per) in forms.items()})
    ms = {k: span([r[k][0] for r in reps]) for k in forms}
    cases = {}
    for key, (m, nrooms, copy, n) in info.items():
        rec = m.records()
        c = {"rooms": nrooms, "talkers_per_room": float(rec[:, 0].sum()) / nrooms, "ms": ms[key],
             "over_copy": span([r[key][0] / r[copy][0] for r in reps]),
             "share_of_tick": span([r[key][0] / (n / 16.0) for r in reps])}
        if not a.no_step:
            c["over_packet_slot_step"] = span([r[key][0] / r["packet_slot_step_16k_160"][0] for r in reps])
        cases[key] = c
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "participants": P,
           "timing": "per repetition: median (min, max) in ms over %d windows of 4 calls (packet-slot step: %d windows of 1), device "
                     "events, warmed; %d repetitions, the forms in turn; the summary is the span of the repetitions' medians"
                     % (a.iters, max(a.iters // 2, 4), a.reps),
           "reps": reps, "ms": ms, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    for key, c in cases.items():
        print("%-28s %8.4f ms  = %6.2f x copy, %6.3f %% of the tick%s" % (
            key, c["ms"]["median"], c["over_copy"]["median"], 100 * c["share_of_tick"]["median"],
            "" if a.no_step else ", %6.3f %% of the packet-slot step" % (100 * c["over_packet_slot_step"]["median"])), flush=True)
    if not a.no_step:
        print("packet-slot step (16 kHz / 160, %d slots): %.3f ms" % (P, ms["packet_slot_step_16k_160"]["median"]))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
