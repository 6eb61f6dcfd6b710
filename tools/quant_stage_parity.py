#!/usr/bin/env python3
"""Measured ratios of the pinned, per-stage check of the int8/fp16 variant (tests/quant_cases.py: accept_stages), from
exactly the inputs of tests/test_gpu_quant_stages.py and tests/test_quant_checker.py -> profiles/quant_stage_parity.json.

Sections (each one replaces its entry in the output file, the others are kept):
  device    the kernels (needs the GPU): per parameter set and stage, mean and worst statistic / floor over the stage
            cases and their seeds, and the worst case
  standins  CPU: the float32 order and the two-halves order each played as the device against a floor made of the OTHER
            one and the pooled floors; the float32 order with the kernels' sigmoid / tanh forms against both (what the
            forms alone cost: it is part of the floor of the stages that hold one)
  mutants   CPU: per seeded bug, the smallest over the stage cases where it is active of its best statistic / floor in
            the stage it is seeded in

  python tools/quant_stage_parity.py --sections standins,mutants
  python tools/quant_stage_parity.py --sections device"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import quant_cases as QC  # noqa: E402

MUTANTS, STAGES = QC.mutants(), QC.stages()

STAT = ("l2", "frame", "frac")


def _ratio(a, f):
    return a / f if f > 0 else (0.0 if a == 0 else float("inf"))


def _summary(rows):
    """rows: [(case name, seed, {stage: ratios})] -> {stage: {mean, worst, worst_case}}."""
    out = {}
    for st in STAGES:
        r = np.array([row[2][st] for row in rows if st in row[2]], np.float64)
        if not len(r):
            continue
        names = [f"{row[0]}/{row[1]}" for row in rows if st in row[2]]
        out[st] = {"mean": [round(float(v), 3) for v in r.mean(axis=0)], "worst": [round(float(v), 3) for v in r.max(axis=0)],
                   "worst_case": names[int(np.argmax(r.max(axis=1)))]}
    return out


def device_section():
    import torch
    from conftest import load_params
    from gtcrn_micro_amd import Engine
    assert torch.cuda.is_available(), "the device section needs the GPU"
    out = {}
    for tag in ("dns3", "rand"):
        eng, rows = Engine(load_params(tag), 0), []
        for case in QC.stage_cases(tag):
            for seed in case.seeds:
                _, rep = QC.accept_stages(QC.device_taps(eng, case, seed), case, seed)
                rows.append((case.name, seed, {st: r[2] for st, r in rep.items()}))
                print(case.name, seed, {st: tuple(round(v, 2) for v in r[2]) for st, r in rep.items()}, flush=True)
        out[tag] = _summary(rows)
    out["device"] = torch.cuda.get_device_name(0)
    return out


def standins_section():
    out = {}
    for tag in ("dns3", "rand"):
        rows = {"f32_vs_split": [], "split_vs_f32": [], "kernel-fn_vs_both": []}
        for case in QC.stage_cases(tag):
            for seed in case.seeds:
                x, taps = case.input(seed), {}
                QC.port(tag, split=True).forward(x, case.in_scale, case.out_scale, taps=taps)
                ref, _, each = QC.pinned_reference(case, x, taps)
                n = {st: ref[st].size for st in ref}
                for key, dev, others in (("f32_vs_split", "f32", ("split",)), ("split_vs_f32", "split", ("f32",)),
                                         ("kernel-fn_vs_both", "kernel-fn", ("f32", "split"))):
                    own = {st: tuple(max(each[o][st][i] for o in others) for i in range(3)) for st in each[dev]}
                    fl = QC.stage_floors(case, own, n)
                    rows[key].append((case.name, seed, {st: tuple(_ratio(a, f) for a, f in zip(each[dev][st], fl[st]))
                                                        for st in each[dev]}))
        out[tag] = {k: _summary(v) for k, v in rows.items()}
    return out


def mutants_section():
    out = {}
    for m, (stage, what) in MUTANTS.items():
        best = None
        for tag in ("dns3", "rand"):
            for case in QC.stage_cases(tag):
                if not QC.mutant_active(m, case):
                    continue
                seed, taps = case.seeds[0], {}
                QC.port(tag, split=True, mutate=m).forward(case.input(seed), case.in_scale, case.out_scale, taps=taps)
                _, rep = QC.accept_stages(taps, case, seed)
                r = max(rep[stage][2])
                if best is None or r < best[0]:
                    best = (r, case.name, STAT[int(np.argmax(rep[stage][2]))])
        out[m] = {"stage": stage, "smallest_best_ratio": round(best[0], 2) if np.isfinite(best[0]) else "inf",
                  "case": best[1], "statistic": best[2]}
        print(m, out[m], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sections", default="standins,mutants")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quant_stage_parity.json"))
    a = ap.parse_args()
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc["K_STAGE"] = QC.K_STAGE
    doc["statistics"] = "ratios statistic / floor in the order rel-L2, worst frame, fraction of differing elements"
    doc["pooled_floors"] = {tag: {st: [float(f"{v:.3e}") for v in p] for st, p in QC.pooled_floors(tag)[0].items()}
                            for tag in ("dns3", "rand")}
    for sec in a.sections.split(","):
        doc[sec] = {"device": device_section, "standins": standins_section, "mutants": mutants_section}[sec]()
    json.dump(doc, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
