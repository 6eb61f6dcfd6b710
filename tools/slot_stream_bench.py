"""Stream slots (gtcrn_wave_stream_step_slots) against the contiguous wave step, at N resident wave streams (default 65 536).

Same process, same GPU, one hop per stream and step, device events over `--iters` steps, warm-up first, the four cases
alternating for `--reps` repetitions; medians:
  (a) the contiguous step of all N streams;
  (b) the indexed step of all N streams, ids in identity order;
  (c) the indexed step of a sorted random half;
  (d) the contiguous step of N / 2 compact streams -- what a caller gets today after paying for compaction.
(b)/(a) is what the indirection costs, (c)/(d) what stepping a subset in place costs against stepping it compacted.

--parent-lib PATH: the regression check of case (a) against the parent commit's library on the same GPU: fresh child
processes, new and parent library alternating, `--reps` each; both medians go into the JSON.
--contiguous-only [--lib PATH]: what such a child runs (case (a) alone, one JSON line).
Writes profiles/slot_stream_bench.json.

--packet-slots: packet stream slots (gtcrn_packet_stream_step_slots) against the contiguous packet form, at 16 384 and 65 536
resident streams (--sizes) and 16 kHz / 160, 16 kHz / 320 and 48 kHz / 480.  One process, the cases alternating, ms per CALL
over one period of 256 / g calls, medians of `--reps` repetitions with their spread:
  contiguous      gtcrn_packet_stream_step of all N streams;
  slots_all       the slot form, all N slots named in identity order, phases equal;
  slots_half      the slot form, a sorted random half, phases staggered over the period (slot s starts s mod period calls late);
  plan_ms         k_packet_plan alone, from the library's launch records (a run of its own), for slots_all and slots_half.
Writes profiles/packet_slots_bench.json.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def engine(lib_path=None):
    from gtcrn_micro_amd import _lib
    if lib_path:
        _lib.LIB_PATH = os.path.abspath(lib_path)
    params = np.fromfile(os.path.join(ROOT, "tests", "golden", "params_dns3.f32"), dtype=np.float32)
    return _lib.Engine(params, 0), torch.hann_window(512).pow(0.5).cuda()


def contiguous_only(a):
    eng, win = engine(a.lib)
    N = a.streams
    eng.reserve(N, 1)
    x = torch.randn(N, 256, device="cuda") * 0.1
    y = torch.empty_like(x)
    st = eng.new_wave_state(N, win)
    step = lambda: eng.wave_stream_step(st, x, out=y)              # noqa: E731
    timed(step, max(3, a.iters // 4))
    t = [timed(step, a.iters) for _ in range(a.reps)]
    print(json.dumps({"lib": a.lib or "default", "N": N, "contiguous_ms": statistics.median(t), "reps_ms": t}), flush=True)


def packet_slots(a):
    from math import gcd
    eng, win = engine()
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "reps": a.reps, "unit": "ms per call over one period",
           "runs": []}
    for N in a.sizes:
        for fs, n in ((16000, 160), (16000, 320), (48000, 480)):
            n16 = n * 16000 // fs
            period = 256 // gcd(n16, 256)
            H = N // 2
            gen = torch.Generator(device="cuda").manual_seed(N + n)
            x = torch.randn(N, n, device="cuda", generator=gen) * 0.1
            y = torch.empty_like(x)
            cs = eng.new_packet_state(N, win, n, fs)
            sa = eng.new_packet_slot_state(N, win, n, fs)
            sh = eng.new_packet_slot_state(N, win, n, fs)
            ident = torch.arange(N, dtype=torch.int32, device="cuda")
            cnt = torch.tensor([N], dtype=torch.int32, device="cuda")
            for k in range(period - 1):                        # stagger: slot s has taken s mod period packets
                late = ident[(ident % period) > k].contiguous()
                if late.numel():
                    eng.packet_stream_step_slots(sh, late, x[:late.numel()], out=y[:late.numel()])
            staggered = sorted(set(sh.phase.tolist()))
            pick = torch.sort(torch.randperm(N, device="cuda", generator=gen)[:H]).values.to(torch.int32)
            cnt_h = torch.tensor([H], dtype=torch.int32, device="cuda")
            xh, yh = x[:H], y[:H]

            def per(fn):
                def run():
                    for _ in range(period):
                        fn()
                return run
            cases = {
                "contiguous": per(lambda: eng.packet_stream_step(cs, x, out=y)),
                "slots_all": per(lambda: eng.packet_stream_step_slots(sa, ident, x, count=cnt, out=y)),
                "slots_half": per(lambda: eng.packet_stream_step_slots(sh, pick, xh, count=cnt_h, out=yh)),
            }
            for f in cases.values():
                timed(f, 1)                                    # warm-up: one period
            t = {k: [] for k in cases}
            for _ in range(a.reps):
                for k, f in cases.items():
                    t[k].append(timed(f, a.iters) / period)
            plan = {}
            for k in ("slots_all", "slots_half"):
                eng.timing_enable(True, only="k_packet_plan")
                cases[k]()
                torch.cuda.synchronize()
                plan[k] = eng.timing_read().get("k_packet_plan", (None, 0))[0]
                eng.timing_enable(False)
            med = {k: statistics.median(v) for k, v in t.items()}
            row = {"N": N, "fs": fs, "n": n, "n16": n16, "period": period, "half": H, "staggered_phases": staggered, "ms": med,
                   "reps_ms": t, "spread": {k: spread(v) for k, v in t.items()}, "plan_ms": plan,
                   "slots_all_over_contiguous": med["slots_all"] / med["contiguous"],
                   "slots_half_per_stream_over_contiguous": (med["slots_half"] / H) / (med["contiguous"] / N)}
            print(json.dumps({k: v for k, v in row.items() if k != "reps_ms"}), flush=True)
            res["runs"].append(row)
            del cs, sa, sh, cases
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slot_stream_bench.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--contiguous-only", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--packet-slots", action="store_true")
    ap.add_argument("--sizes", type=int, nargs="+", default=[16384, 65536])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("slot_stream_bench needs the GPU (nothing is measured on the CPU)")
    if a.contiguous_only:
        return contiguous_only(a)
    if a.packet_slots:
        if a.out.endswith("slot_stream_bench.json"):
            a.out = os.path.join(ROOT, "profiles", "packet_slots_bench.json")
        return packet_slots(a)
    eng, win = engine()
    N, H = a.streams, a.streams // 2
    eng.reserve(N, 1)
    gen = torch.Generator(device="cuda").manual_seed(N)
    x = torch.randn(N, 256, device="cuda", generator=gen) * 0.1
    y = torch.empty_like(x)
    st = eng.new_wave_state(N, win)
    half = eng.new_wave_state(H, win)
    ident = torch.arange(N, dtype=torch.int32, device="cuda")
    pick = torch.sort(torch.randperm(N, device="cuda", generator=gen)[:H]).values.to(torch.int32)
    cnt_all, cnt_half = torch.tensor([N], dtype=torch.int32, device="cuda"), torch.tensor([H], dtype=torch.int32, device="cuda")
    xh, yh = x[:H], y[:H]
    cases = {
        "a_contiguous_all": lambda: eng.wave_stream_step(st, x, out=y),
        "b_indexed_all_identity": lambda: eng.wave_stream_step_slots(st, ident, x, count=cnt_all, out=y),
        "c_indexed_sorted_half": lambda: eng.wave_stream_step_slots(st, pick, xh, count=cnt_half, out=yh),
        "d_contiguous_half_compact": lambda: eng.wave_stream_step(half, xh, out=yh),
    }
    for f in cases.values():
        timed(f, max(3, a.iters // 4))                             # warm-up
    t = {k: [] for k in cases}
    for _ in range(a.reps):
        for k, f in cases.items():
            t[k].append(timed(f, a.iters))
    med = {k: statistics.median(v) for k, v in t.items()}
    res = {"device": torch.cuda.get_device_name(0), "N": N, "half": H, "iters": a.iters, "reps": a.reps,
           "ms": med, "reps_ms": t, "spread": {k: spread(v) for k, v in t.items()},
           "b_over_a": med["b_indexed_all_identity"] / med["a_contiguous_all"],
           "c_over_d": med["c_indexed_sorted_half"] / med["d_contiguous_half_compact"]}
    print(json.dumps({k: v for k, v in res.items() if k != "reps_ms"}), flush=True)
    del st, half, cases
    torch.cuda.empty_cache()
    if a.parent_lib:
        runs = {"new": [], "parent": []}
        for _ in range(2):
            for tag, lib in (("new", None), ("parent", a.parent_lib)):
                cmd = [sys.executable, os.path.abspath(__file__), "--contiguous-only", "--streams", str(N), "--iters", str(a.iters),
                       "--reps", str(a.reps)] + (["--lib", lib] if lib else [])
                out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300).stdout
                runs[tag].append(json.loads(out.strip().splitlines()[-1])["contiguous_ms"])
        res["parent_check"] = {"new_ms": statistics.median(runs["new"]), "parent_ms": statistics.median(runs["parent"]),
                               "new_runs_ms": runs["new"], "parent_runs_ms": runs["parent"]}
        res["parent_check"]["new_over_parent"] = res["parent_check"]["new_ms"] / res["parent_check"]["parent_ms"]
        print(json.dumps(res["parent_check"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
