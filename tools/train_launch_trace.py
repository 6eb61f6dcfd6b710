#!/usr/bin/env python3
"""Which kernels the training launch layer picks: one train step per configuration, to be run under a kernel trace,
and the comparison of two such traces.

A launcher of train_kernels.hip that picks a general instantiation where a specialised one was meant computes the
same bits, only slower: no test sees it.  The launch sequence does.  A step runs on one stream, so two builds of the
library that make the same decisions give the same ordered list of (kernel, grid, workgroup, LDS bytes).

    rocprofv3 --kernel-trace --output-format csv -d OUT/new -- python3 tools/train_launch_trace.py run
    GTCRN_LIB_VARIANT=exp rocprofv3 --kernel-trace --output-format csv -d OUT/old -- python3 tools/train_launch_trace.py run
    python3 tools/train_launch_trace.py compare OUT/old OUT/new --kernels profiles/train_launch_dispatch_asm.txt \
            --out profiles/train_launch_dispatch_trace.json

(the other build sits in the GT_EXP slot, gtcrn_micro_amd/libgtcrn_micro_hip_exp.so: see _lib.lib()).  Each traced run
is a process of its own; no counters are collected.  `run` walks storage mode x fusion mask x (B, T) on frame-major
spectrograms -- the train step's own layout; without the two masks the trainer refuses for bf16_grads -- and every storage mode at (B, T) on a time-major and on a misaligned
spectrogram, so that all three layout forms of feat_fwd / bs_mask_fwd / bs_mask_bwd launch.  A configuration is one
step: forward, HybridLoss, backward, clip + Adam.  `compare` exits 1 unless the two sequences are equal element for
element; --kernels (an asm_compare.py listing) adds the kernels of the file that no configuration launched."""
import argparse
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STORAGES = ("f32", "bf16", "bf16_saves", "bf16_grads")
MASKS = (65535, 16383, 8191, 1023, 7, 0)
SHAPES = ((2, 24), (5, 13))          # tests/test_gpu_train.py, test_tile_kernels_at_odd_shapes_...


def configs():
    # (the trainer itself refuses bf16 gradient hand-offs without fusion bit 4, the in-place skip gradients: masks 7 and 0)
    out = [(st, m, bt, "frame_major") for st in STORAGES for m in MASKS for bt in SHAPES if st != "bf16_grads" or m & 16]
    out += [(st, 65535, bt, lay) for lay in ("time_major", "misaligned") for st in STORAGES for bt in SHAPES]
    return out


def spectrogram(B, T, layout, gen):
    import torch
    if layout == "time_major":        # torch.stft's layout: the frame axis fastest
        return torch.randn(B, 257, T, 2, device="cuda", generator=gen) * 0.5
    if layout == "frame_major":
        return (torch.randn(B, T, 257, 2, device="cuda", generator=gen) * 0.5).permute(0, 2, 1, 3)
    # frame-major strides behind a base that is 4 but not 8 bytes aligned: neither special form takes it
    buf = torch.randn(B * T * 514 + 1, device="cuda", generator=gen) * 0.5
    return buf[1:].view(B, T, 257, 2).permute(0, 2, 1, 3)


def run():
    import numpy as np
    import torch
    import gtcrn_micro_amd as G
    import gtcrn_micro_amd._lib as L
    blob_np = np.fromfile(os.path.join(ROOT, "tests", "golden", "params_rand.f32"), np.float32)
    mask_adam = torch.ones(L.NPARAM_FLOATS, device="cuda")
    refused = []
    for storage, fusions, (B, T), layout in configs():
        gen = torch.Generator("cuda").manual_seed(B * 100 + T)
        spec = spectrogram(B, T, layout, gen)
        true = spectrogram(B, T, "frame_major" if layout == "misaligned" else layout, gen)   # (the loss sees the output's layout)
        blob = torch.from_numpy(blob_np.copy()).cuda()
        m, v = torch.zeros_like(blob), torch.zeros_like(blob)
        tr = G.Trainer(0)
        tr.set_storage(storage)
        tr.set_fusions(fusions)
        try:
            out = tr.forward(blob, spec)
            loss, gout = tr.hybrid_loss(out, true)
            grads = tr.backward(blob, spec, gout)
            L.clip_adam_step(blob, grads, m, v, mask_adam, 1, 1e-3, max_norm=3.0)
        except L.GtcrnError as e:      # a refusal is an answer too (both builds must give it); a fault ends the run below
            refused.append(f"{storage} {fusions} {B}x{T} {layout}: {e}")
            torch.cuda.synchronize()
            tr.close()
            continue
        torch.cuda.synchronize()
        if not bool(torch.isfinite(loss)) or not bool(torch.isfinite(grads).all()):
            raise SystemExit(f"non-finite step at {storage} {fusions} {B}x{T} {layout}")
        tr.close()
    print(json.dumps({"configurations": len(configs()), "refused": refused,
                      "library": os.environ.get("GTCRN_LIB_VARIANT") or "default"}))


def short_name(name):
    """The kernel's name as tools/asm_compare.py prints it: demangled, without the argument list."""
    name = re.sub(r"\.kd$", "", name.strip()).replace("(anonymous namespace)", "{anonymous}")
    return re.sub(r"\(.*$", "", name).replace("void ", "", 1).strip()


def dispatches(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"{trace_dir}: expected one *kernel_trace.csv, found {len(files)}")
    rows = list(csv.DictReader(open(files[0], newline="")))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    return [(short_name(r["Kernel_Name"]), tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ"),
             tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"), int(r["LDS_Block_Size"])) for r in rows]


def compare(a):
    old, new = dispatches(a.old), dispatches(a.new)
    first = next((i for i, (x, y) in enumerate(zip(old, new)) if x != y), None)
    if first is None and len(old) != len(new):
        first = min(len(old), len(new))
    launched = {}
    for d in new:
        launched[d[0]] = launched.get(d[0], 0) + 1
    res = {"what": "ordered (kernel, grid, workgroup, LDS bytes) of one train step per configuration, parent library "
                   "against this tree's, rocprofv3 --kernel-trace, one process each",
           "configurations": [{"storage": s, "fusions": m, "B": bt[0], "T": bt[1], "layout": lay} for s, m, bt, lay in configs()],
           "dispatches_old": len(old), "dispatches_new": len(new), "equal": first is None,
           "first_difference": None if first is None else
           {"index": first, "old": old[first] if first < len(old) else None, "new": new[first] if first < len(new) else None}}
    if a.kernels:
        names = [short_name(ln.split(None, 2)[2]) for ln in open(a.kernels) if ln.startswith("same ")]
        res["kernels_in_file"] = len(names)
        res["kernels_launched"] = sum(1 for n in names if n in launched)
        res["launch_counts"] = {n: launched[n] for n in sorted(names) if n in launched}
        res["never_launched"] = sorted(n for n in names if n not in launched)
        res["never_launched_note"] = ("no traced configuration reaches these instantiations: for the branches that pick "
                                      "them the evidence is the reading of the launchers alone")
    text = json.dumps(res, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(json.dumps({k: res[k] for k in ("dispatches_old", "dispatches_new", "equal", "first_difference")}))
    if a.kernels:
        print(f"{res['kernels_launched']} of {res['kernels_in_file']} kernels launched")
    return 0 if first is None else 1


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("run")
    c = sub.add_parser("compare")
    c.add_argument("old")
    c.add_argument("new")
    c.add_argument("--kernels", default=None)
    c.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.cmd == "run":
        run()
        return 0
    return compare(a)


if __name__ == "__main__":
    sys.exit(main())
