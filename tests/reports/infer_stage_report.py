#!/usr/bin/env python3
"""Diagnostic (GPU box): the fp32 inference path stage by stage against the pinned float64 checker
(oracle/infer_pinned.py).  Everything the margins in infer_pinned.MARGINS and DESIGN.md cite is in the file it writes:

  cases             per stage and parameter set, at (B, T) = (2, 33) and (1, 90): the table of infer_pinned.measure, the
                    HIP / float32-port ratios (worst channel; raw and net of the slope allowance) and "fold", the float64
                    graph on the packer's folded constants over the port (infer_pinned.CONSTS)
  worst_over_cases  the worst of those ratios, per stage, over every case of tests/test_gpu_infer_pinned.py, with the case
  en1_chain         en_convs.1 as one fp32 chain on the CPU (infer_pinned.simulate_en1_chain) beside the device, in the
                    device's worst channel, over the port's worst channel
  bugs              how far every seeded wrong layer is rejected on the HIP taps (failing figure / bound)

Nothing in the suite reads the file.

    python tests/reports/infer_stage_report.py [--out profiles/infer_stage_pinned.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from gtcrn_micro_amd import Engine                      # noqa: E402
from oracle import infer_pinned as IP                   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infer_stage_pinned.json"))
args = ap.parse_args()
torch.set_num_threads(min(8, torch.get_num_threads()))
SHAPES = [(2, T) for T in (1, 2, 5, 6, 10, 11, 16, 17, 33)] + [(1, 90), (5, 40)]      # tests/test_gpu_infer_pinned.py
TABLE = ((2, 33), (1, 90))
report = {"margins": {"default": IP.DEFAULT_MARGIN, **IP.MARGINS}, "abs_floor": IP.ABS_FLOOR,
          "figures": "error / channel rms in the float64 checker (out: per band of 16 bins); ratios are HIP worst channel / "
                     "float32 port worst channel, [rms, max]; net: the slope allowance of the channel furthest over its "
                     "bound taken off the HIP figure first",
          "cases": [], "worst_over_cases": {}, "en1_chain": [], "bugs": []}
worst = {s: {"raw": [[0.0, ""], [0.0, ""]], "net": [[0.0, ""], [0.0, ""]]} for s in IP.STAGES}
for tag in ("dns3", "rand"):
    blob = np.fromfile(os.path.join(ROOT, "tests", "golden", f"params_{tag}.f32"), np.float32)
    eng = Engine(blob, 0)
    eng.debug_enable(True)
    for kind in ("white", "tilt"):
        for B, T in SHAPES:
            case = f"{tag} {kind} {B}x{T}"
            spec = IP.make_input(kind, B, T, seed=100 * B + T)
            out = eng.forward_spec(torch.from_numpy(spec).cuda()).cpu().numpy()
            taps = IP.engine_taps(eng, B, T)
            IP.check_sum4(taps)
            clean = IP.pinned_run(blob, spec, taps)
            yard = IP.yardstick(blob, spec, taps, clean)
            rows = IP.measure(blob, spec, taps, out, yard=yard)
            rt = IP.ratios(rows)
            print(f"{case}: {IP.summary(rows)}", flush=True)
            for s, (raw, net) in rt.items():
                for k in range(2):
                    for key, v in (("raw", raw[k]), ("net", net[k])):
                        if s != "de4" or key == "raw":      # (de4's bound is the absolute allowance: no net figure)
                            if v > worst[s][key][k][0]:
                                worst[s][key][k] = [v, case]
            if (B, T) not in TABLE:
                continue
            fold = IP._as_got(IP.pinned_run(blob, spec, taps, consts="fold"), taps)
            ff = {}
            for s in IP.STAGES:
                fg, pg = IP.stage_figures(s, fold, clean, taps), yard["port"][s]
                ff[s] = [float(fg[k].max() / pg[k].max()) for k in range(2)]
            for r in rows:
                print("   " + IP.fmt(r) + ("" if r.ok else "   <-- above the bound"))
            report["cases"].append({"params": tag, "input": kind, "B": B, "T": T,
                                    "ratios": {s: {"raw": rt[s][0], "net": rt[s][1], "fold": ff[s]} for s in IP.STAGES},
                                    "rows": [dict(r._asdict(), **{"class": r.cls}) for r in rows]})
            if (B, T) == (2, 33):
                h = IP.stage_figures("en1", dict(taps, out=out), clean, taps)[0]
                b, c = np.unravel_index(int(np.argmax(h)), h.shape)
                den = np.sqrt((clean["en1"][b, c] ** 2).mean())
                sim = {}
                for name, order, seed in (("kernel", "kernel", 0), ("random0", "random", 0), ("random1", "random", 1),
                                          ("shift_last", "shift_last", 0)):
                    y = IP.simulate_en1_chain(blob, taps["en0"], order, seed)[b, c].astype(np.float64)
                    sim[name] = float(np.sqrt(((y - clean["en1"][b, c]) ** 2).mean()) / den)
                pw = float(yard["port"]["en1"][0].max())
                print(f"   en1 clip {b} channel {c}: HIP {h[b, c]:.3e}, port's worst channel {pw:.3e}; one fp32 chain on "
                      f"the CPU: " + ", ".join(f"{k} {v:.3e} ({v / pw:.2f}x)" for k, v in sim.items()))
                report["en1_chain"].append({"params": tag, "input": kind, "B": B, "T": T, "clip": int(b), "channel": int(c),
                                            "hip": float(h[b, c]), "port_worst": pw, "chain": sim})
    spec = IP.make_input("white", 2, 33, seed=7)        # the input of the tests' seeded-bug case
    out = eng.forward_spec(torch.from_numpy(spec).cuda()).cpu().numpy()
    taps = IP.engine_taps(eng, 2, 33)
    yard = IP.yardstick(blob, spec, taps)
    for bug, (stage, what) in IP.BUGS.items():
        brows = IP.measure(blob, spec, taps, out, bug=bug, yard=yard)
        d = IP.distance(brows, stage)
        print(f"   bug {bug} ({what}): rejected at {IP.failing_stages(brows)}, {d:.3g}x the bound")
        report["bugs"].append({"params": tag, "bug": bug, "stage": stage, "what": what,
                               "rejected_at": IP.failing_stages(brows), "figure_over_bound": d})
report["worst_over_cases"] = worst
print("worst over cases, net of the slope allowance (rms | max): " + " ".join(
    f"{s} {w['net'][0][0]:.2f}|{w['net'][1][0]:.2f}" for s, w in worst.items()))
with open(args.out, "w") as f:
    json.dump(report, f, indent=1)
print("wrote", args.out)
