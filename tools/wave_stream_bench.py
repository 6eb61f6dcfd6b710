"""Hop-level waveform streaming (gtcrn_wave_stream_step) against the spectral step (gtcrn_stream_step) it wraps.

Same process, same GPU: for each stream count N, one hop (wave: 256 samples in / out; spectral: one 257-bin frame in /
out) per stream and step, timed with device events over `--iters` steps, warm-up first, the two sides alternating for
`--reps` repetitions; medians.  Also the per-call latency at N = 1, eager and under graph replay, and the compulsory
bytes the two wave kernels add per stream-step (from shapes).  Writes profiles/wave_stream_bench.json.

--trace-only N: just run wave steps at N streams (for `rocprofv3 --kernel-trace --stats -- python <this> --trace-only N`).

--rate: the step at the caller's rate (gtcrn_rate_stream_step: k_rate_in, the wave step, k_rate_out) at 48 kHz and 8 kHz
against the 16 kHz wave step of the SAME run, same warm-up, repetitions and medians; writes
profiles/rate_stream_bench.json.  With --trace-only N: rate steps at --trace-fs (default 48000).

--rate --highband: the high band.  At 16 384 and 65 536 streams (or --sizes), 48 kHz, the plain rate step and the rate step
of a state with highband=0.5 (gtcrn_rate_stream_step_hb: k_rate_out_hb as the fifth launch) alternate in one run; each
figure stands next to that run's own repetition spread.  Writes profiles/highband_rate_bench.json.

--packet: the packet form (gtcrn_packet_stream_step) at 16 384 and 65 536 streams (or --sizes): 16 kHz / 160 and 320,
48 kHz / 480, 44.1 kHz / 441.  The timed unit is one whole period of calls, divided by the hops it steps, next to the
per-hop time of the 16 kHz wave step and the 48 kHz rate step of the SAME run; plus every call of a period on its own
(the cost follows the hops of the call) and the library's per-kernel event times over one period.  Writes
profiles/packet_stream_bench.json.  With --trace-only N: packet steps at --trace-fs / --trace-packet.

--packet --highband: the high band on the packet form.  At 16 384 and 65 536 streams (or --sizes), 48 kHz / 480 and 48 kHz /
960, one whole period of the plain packet call and of the call of a state with highband=0.5 (gtcrn_packet_stream_step_hb:
k_packet_out_hb in the place of k_packet_out) alternate in one run; each ratio stands next to that run's own repetition
spread, the plain figure next to the one profiles/packet_stream_bench.json holds for the same case, and the outbound
kernel's own event times of both forms come from the library's launch records.  Writes profiles/highband_packet_bench.json.

--dry-gain: the attenuation limit.  At 16 384 and 65 536 streams (or --sizes) the plain and the limited 16 kHz wave step
(12 dB on every stream) alternate in one run, then one period of the plain and the limited packet form at 16 kHz / 160;
offline, the library's event times of k_istft and k_istft_mix at B = 256 x 4 s.  Each limited figure stands next to the
plain one of the SAME run and that run's own repetition spread.  Writes profiles/dry_gain_bench.json.  With
--trace-only N: plain and limited wave steps alternating, then plain and limited offline calls (for one rocprofv3
--kernel-trace --stats run that holds k_wave_synthesis and k_istft in both forms).

--meters: the level meters.  At 16 384 and 65 536 streams (or --sizes) the plain and the metered 16 kHz wave step alternate
in one run, then one period of the plain and the metered packet form at 16 kHz / 160, as --dry-gain does; the library's
event times of k_wave_synthesis against k_wave_synthesis_meter come from that run's launch records.  Each metered figure
stands next to the plain one of the SAME run and that run's own repetition spread.  Writes profiles/meters_bench.json.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def traffic_per_stream_step(sample_bytes=4):
    """Compulsory DRAM bytes the analysis + synthesis kernels add to one single-hop step of one stream."""
    spec = 257 * 2 * 4
    analysis = {"input hop": 256 * sample_bytes, "ring (previous hop)": 256 * 4, "hop counter": 4, "spectrum out": spec}
    synthesis = {"spectrum in": spec, "tail in": 256 * 4, "ring (newest half) in": 256 * 4, "input hop": 256 * sample_bytes,
                 "hop counter": 8, "output hop": 256 * sample_bytes, "tail out": 256 * 4, "ring out": 512 * 4}
    return {"analysis": analysis, "synthesis": synthesis,
            "total_bytes": sum(analysis.values()) + sum(synthesis.values())}


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def compare(eng, win, N, iters, reps):
    from gtcrn_micro_amd._lib import empty_spec
    eng.reserve(N, 1)
    gen = torch.Generator(device="cuda").manual_seed(N)
    x = torch.randn(N, 256, device="cuda", generator=gen) * 0.1
    y = torch.empty_like(x)
    spec = empty_spec(N, 1, "cuda", frame_major=True)
    spec.copy_(torch.randn(spec.shape, device="cuda", generator=gen) * 0.3)
    sout = empty_spec(N, 1, "cuda", frame_major=True)
    sst = eng.new_state(N)
    wst = eng.new_wave_state(N, win)
    spectral = lambda: eng.stream_step(sst, spec, out=sout)       # noqa: E731
    wave = lambda: eng.wave_stream_step(wst, x, out=y)            # noqa: E731
    for f in (spectral, wave):
        timed(f, max(3, iters // 4))                              # warm-up
    ts, tw = [], []
    for _ in range(reps):
        ts.append(timed(spectral, iters))
        tw.append(timed(wave, iters))
    ms_s, ms_w = statistics.median(ts), statistics.median(tw)
    del sst, wst
    torch.cuda.empty_cache()
    return {"N": N, "spectral_step_ms": ms_s, "wave_step_ms": ms_w, "ratio": ms_w / ms_s,
            "spectral_reps_ms": ts, "wave_reps_ms": tw, "iters": iters}


def compare_rate(eng, win, N, iters, reps, rates=(48000, 8000)):
    """One hop per stream and step: the 16 kHz wave step and the rate step at each of `rates`, alternating."""
    gen = torch.Generator(device="cuda").manual_seed(N)
    x = torch.randn(N, 256, device="cuda", generator=gen) * 0.1
    y = torch.empty_like(x)
    eng.reserve(N, 1)
    wst = eng.new_wave_state(N, win)
    fns = {16000: lambda: eng.wave_stream_step(wst, x, out=y)}
    keep = [wst]
    for fs in rates:
        st = eng.new_rate_state(N, win, fs)
        eng.rate_stream_reserve(st, 1)
        xr = torch.randn(N, st.hop, device="cuda", generator=gen) * 0.1
        yr = torch.empty_like(xr)
        fns[fs] = lambda st=st, xr=xr, yr=yr: eng.rate_stream_step(st, xr, out=yr)
        keep.append(st)
    for f in fns.values():
        timed(f, max(3, iters // 4))                              # warm-up
    t = {fs: [] for fs in fns}
    for _ in range(reps):
        for fs, f in fns.items():
            t[fs].append(timed(f, iters))
    med = {fs: statistics.median(v) for fs, v in t.items()}
    del keep, fns
    torch.cuda.empty_cache()
    r = {"N": N, "wave_step_16k_ms": med[16000], "wave_reps_16k_ms": t[16000], "iters": iters}
    for fs in rates:
        r[f"rate_step_{fs}_ms"] = med[fs]
        r[f"ratio_{fs}"] = med[fs] / med[16000]
        r[f"rate_reps_{fs}_ms"] = t[fs]
    return r


def compare_highband(eng, win, N, iters, reps, fs=48000, gain=0.5):
    """One hop per stream and step at `fs`: the plain rate step and the step with the high band, alternating."""
    gen = torch.Generator(device="cuda").manual_seed(N)
    sp, sh = eng.new_rate_state(N, win, fs), eng.new_rate_state(N, win, fs, highband=gain)
    eng.rate_stream_reserve(sp, 1)
    x = torch.randn(N, sp.hop, device="cuda", generator=gen) * 0.1
    y = torch.empty_like(x)
    plain = lambda: eng.rate_stream_step(sp, x, out=y)             # noqa: E731
    hb = lambda: eng.rate_stream_step(sh, x, out=y)                # noqa: E731
    for f in (plain, hb):
        timed(f, max(3, iters // 4))                              # warm-up
    tp, th = [], []
    for _ in range(reps):
        tp.append(timed(plain, iters))
        th.append(timed(hb, iters))
    r = {"N": N, "fs": fs, "highband": gain, "iters": iters, "rate_step_plain_ms": statistics.median(tp),
         "rate_step_highband_ms": statistics.median(th), "rate_step_plain_reps_ms": tp, "rate_step_highband_reps_ms": th,
         "rate_step_plain_spread": spread(tp), "rate_step_highband_spread": spread(th),
         "highband_state_bytes_per_stream": sh.hb.shape[1] * 4}
    r["ratio"] = r["rate_step_highband_ms"] / r["rate_step_plain_ms"]
    del sp, sh
    torch.cuda.empty_cache()
    return r


PACKET_CASES = ((16000, 160), (16000, 320), (48000, 480), (44100, 441))


def compare_packet(eng, win, N, iters, reps, cases=PACKET_CASES):
    """The packet form (gtcrn_packet_stream_step) at N streams: for each (fs, packet) one WHOLE PERIOD of calls is the
    timed unit (its launch sequence repeats from there), divided by the hops it steps; next to it the per-hop time of
    the 16 kHz wave step and of the 48 kHz rate step, alternating in the same run.  Then, per case: every call of a
    period timed on its own (the cost follows the hops h of the call) and the library's per-kernel event times."""
    gen = torch.Generator(device="cuda").manual_seed(N)
    eng.reserve(N, 1)
    x = torch.randn(N, 256, device="cuda", generator=gen) * 0.1
    y = torch.empty_like(x)
    wst = eng.new_wave_state(N, win)
    rst = eng.new_rate_state(N, win, 48000)
    eng.rate_stream_reserve(rst, 1)
    xr = torch.randn(N, rst.hop, device="cuda", generator=gen) * 0.1
    yr = torch.empty_like(xr)
    wave = lambda: eng.wave_stream_step(wst, x, out=y)             # noqa: E731
    rate = lambda: eng.rate_stream_step(rst, xr, out=yr)           # noqa: E731
    res = {"N": N, "iters": iters, "cases": []}
    tw, tr = [], []
    for fs, n in cases:
        st = eng.new_packet_state(N, win, n, fs)
        P = st.period
        xp = torch.randn(N, n, device="cuda", generator=gen) * 0.1
        yp = torch.empty_like(xp)
        hops = []

        def period():
            for _ in range(P):
                eng.packet_stream_step(st, xp, out=yp)

        for _ in range(P):
            hops.append(st.next_hops)
            eng.packet_stream_step(st, xp, out=yp)
        nper = max(2, iters // P)
        for f in (wave, rate):
            timed(f, max(3, iters // 4))                           # warm-up (every h of the period ran above)
        timed(period, 2)
        tp, w, r = [], [], []
        for _ in range(reps):
            w.append(timed(wave, iters))
            r.append(timed(rate, iters))
            tp.append(timed(period, nper))
        tw += w
        tr += r
        # every call of a period on its own
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(P + 1)] for _ in range(nper)]
        for k in range(nper):
            ev[k][0].record()
            for p in range(P):
                eng.packet_stream_step(st, xp, out=yp)
                ev[k][p + 1].record()
        torch.cuda.synchronize()
        per_call = [statistics.median(ev[k][p].elapsed_time(ev[k][p + 1]) for k in range(nper)) for p in range(P)]
        eng.timing_enable(True)
        period()
        torch.cuda.synchronize()
        kern = {k: {"avg_ms": v[0], "launches": v[1]} for k, v in eng.timing_read().items()}
        eng.timing_enable(False)
        ms_period = statistics.median(tp)
        c = {"fs": fs, "packet": n, "n16": st.n16, "period_calls": P, "hops_per_period": sum(hops), "hops_by_call": hops,
             "latency16": st.latency16, "period_ms": ms_period, "per_hop_ms": ms_period / sum(hops),
             "per_call_ms": ms_period / P, "period_reps_ms": tp, "wave_per_hop_ms": statistics.median(w),
             "rate48k_per_hop_ms": statistics.median(r), "call_ms_by_position": per_call, "kernels_one_period": kern,
             "packet_kernel_bytes_per_stream_call": 8 * (st.n16 + 256 * sum(hops) / P)}
        c["per_hop_vs_wave"] = c["per_hop_ms"] / c["wave_per_hop_ms"]
        c["per_hop_vs_rate48k"] = c["per_hop_ms"] / c["rate48k_per_hop_ms"]
        res["cases"].append(c)
        del st
        torch.cuda.empty_cache()
    res["wave_step_16k_ms"] = statistics.median(tw)
    res["rate_step_48000_ms"] = statistics.median(tr)
    del wst, rst
    torch.cuda.empty_cache()
    return res


HIGHBAND_PACKET_CASES = ((48000, 480), (48000, 960))


def compare_packet_highband(eng, win, N, iters, reps, cases=HIGHBAND_PACKET_CASES, gain=0.5):
    """One whole period of the plain packet call and of the call with the high band at N streams, alternating."""
    gen = torch.Generator(device="cuda").manual_seed(N)
    earlier = {}
    try:
        with open(os.path.join(ROOT, "profiles", "packet_stream_bench.json")) as f:
            for r in json.load(f)["compare"]:
                if r["N"] == N:
                    earlier = {(c["fs"], c["packet"]): c["period_ms"] for c in r["cases"]}
    except (OSError, KeyError, ValueError):
        pass
    res = {"N": N, "iters": iters, "highband": gain, "cases": []}
    for fs, n in cases:
        sp, sh = eng.new_packet_state(N, win, n, fs), eng.new_packet_state(N, win, n, fs, highband=gain)
        P = sp.period
        x = torch.randn(N, n, device="cuda", generator=gen) * 0.1
        y = torch.empty_like(x)

        def period(st):
            for _ in range(P):
                eng.packet_stream_step(st, x, out=y)

        hops = []
        for _ in range(P):
            hops.append(sp.next_hops)
            eng.packet_stream_step(sp, x, out=y)
        period(sh)                                                 # (every h of the period ran on both states)
        nper = max(2, iters // P)
        for st in (sp, sh):
            timed(lambda: period(st), 2)
        tp, th = [], []
        for _ in range(reps):
            tp.append(timed(lambda: period(sp), nper))
            th.append(timed(lambda: period(sh), nper))
        kern = {}
        for tag, st in (("plain", sp), ("highband", sh)):
            eng.timing_enable(True)
            period(st)
            torch.cuda.synchronize()
            kern[tag] = {k: {"avg_ms": v[0], "launches": v[1]} for k, v in eng.timing_read().items()}
            eng.timing_enable(False)
        c = {"fs": fs, "packet": n, "n16": sp.n16, "period_calls": P, "hops_per_period": sum(hops), "hops_by_call": hops,
             "latency_samples": sh.hb_latency, "highband_state_bytes_per_stream": sh.hb.shape[1] * 4,
             "period_plain_ms": statistics.median(tp), "period_highband_ms": statistics.median(th),
             "period_plain_reps_ms": tp, "period_highband_reps_ms": th, "period_plain_spread": spread(tp),
             "period_highband_spread": spread(th), "period_plain_ms_in_packet_stream_bench": earlier.get((fs, n)),
             "k_packet_out_ms": kern["plain"]["k_packet_out"]["avg_ms"],
             "k_packet_out_hb_ms": kern["highband"]["k_packet_out"]["avg_ms"], "kernels_one_period": kern}
        c["ratio"] = c["period_highband_ms"] / c["period_plain_ms"]
        c["k_packet_out_ratio"] = c["k_packet_out_hb_ms"] / c["k_packet_out_ms"]
        # what the two delay lines move per stream and call: read and written once each
        c["delay_line_bytes_per_stream_call"] = 2 * c["highband_state_bytes_per_stream"]
        res["cases"].append(c)
        del sp, sh
        torch.cuda.empty_cache()
    return res


def spread(v):
    """(max - min) / median of the repetitions of one side: the run's own noise."""
    return (max(v) - min(v)) / statistics.median(v)


def compare_dry_gain(eng, win, N, iters, reps, db=12.0, packet=160):
    """Plain against limited at N streams (compare_pair)."""
    return compare_pair(eng, win, N, iters, reps, "limited", {"atten_lim_db": db}, packet)


def compare_meters(eng, win, N, iters, reps, packet=160):
    """Plain against metered at N streams (compare_pair), plus the synthesis kernels' own event times side by side."""
    r = compare_pair(eng, win, N, iters, reps, "metered", {"meters": True}, packet)
    k = r["kernels_event_timed"]
    r["k_wave_synthesis_ms"], r["k_wave_synthesis_meter_ms"] = k["k_wave_synthesis"]["avg_ms"], k["k_wave_synthesis_meter"]["avg_ms"]
    r["k_wave_synthesis_ratio"] = r["k_wave_synthesis_meter_ms"] / r["k_wave_synthesis_ms"]
    return r


def compare_pair(eng, win, N, iters, reps, tag, kw, packet):
    """Plain against the states made with `kw` (keys named `tag`) at N streams, alternating in one run: the one-hop 16 kHz
    wave step, then one whole period of the packet form at 16 kHz / `packet`."""
    gen = torch.Generator(device="cuda").manual_seed(N)
    eng.reserve(N, 1)
    x = torch.randn(N, 256, device="cuda", generator=gen) * 0.1
    y = torch.empty_like(x)
    sp, sl = eng.new_wave_state(N, win), eng.new_wave_state(N, win, **kw)
    plain = lambda: eng.wave_stream_step(sp, x, out=y)             # noqa: E731
    lim = lambda: eng.wave_stream_step(sl, x, out=y)               # noqa: E731
    for f in (plain, lim):
        timed(f, max(3, iters // 4))
    tp, tl = [], []
    for _ in range(reps):
        tp.append(timed(plain, iters))
        tl.append(timed(lim, iters))
    eng.timing_enable(True)
    for _ in range(iters):
        plain()
        lim()
    torch.cuda.synchronize()
    kern = {k: {"avg_ms": v[0], "launches": v[1]} for k, v in eng.timing_read().items()}
    eng.timing_enable(False)
    r = {"N": N, "iters": iters, **kw, "wave_step_plain_ms": statistics.median(tp),
         f"wave_step_{tag}_ms": statistics.median(tl), "wave_step_plain_reps_ms": tp, f"wave_step_{tag}_reps_ms": tl,
         "wave_step_plain_spread": spread(tp), f"wave_step_{tag}_spread": spread(tl), "kernels_event_timed": kern}
    r["wave_step_ratio"] = r[f"wave_step_{tag}_ms"] / r["wave_step_plain_ms"]
    del sp, sl
    torch.cuda.empty_cache()
    pp, pl = eng.new_packet_state(N, win, packet), eng.new_packet_state(N, win, packet, **kw)
    P = pp.period
    xp = torch.randn(N, packet, device="cuda", generator=gen) * 0.1
    yp = torch.empty_like(xp)

    def period(st):
        for _ in range(P):
            eng.packet_stream_step(st, xp, out=yp)

    nper = max(2, iters // P)
    for st in (pp, pl):
        timed(lambda: period(st), 2)
    qp, ql = [], []
    for _ in range(reps):
        qp.append(timed(lambda: period(pp), nper))
        ql.append(timed(lambda: period(pl), nper))
    r.update({"packet": packet, "period_calls": P, "packet_period_plain_ms": statistics.median(qp),
              f"packet_period_{tag}_ms": statistics.median(ql), "packet_period_plain_reps_ms": qp,
              f"packet_period_{tag}_reps_ms": ql, "packet_period_plain_spread": spread(qp),
              f"packet_period_{tag}_spread": spread(ql)})
    r["packet_period_ratio"] = r[f"packet_period_{tag}_ms"] / r["packet_period_plain_ms"]
    del pp, pl
    torch.cuda.empty_cache()
    return r


def offline_dry_gain(eng, win, B=256, seconds=4, reps=7, db=12.0):
    """k_istft against k_istft_mix at B clips of `seconds` s, from the library's launch records (alternating calls)."""
    from gtcrn_micro_amd import atten_lim_to_gain
    L = 16000 * seconds
    x = torch.randn(B, L, device="cuda") * 0.1
    y = torch.empty(B, 256 * (L // 256), device="cuda")
    g = torch.full((B,), atten_lim_to_gain(db), device="cuda")
    for _ in range(2):
        eng.forward_wave(x, win, out=y)
        eng.forward_wave(x, win, out=y, dry_gain=g)
    eng.timing_enable(True)
    for _ in range(reps):
        eng.forward_wave(x, win, out=y)
        eng.forward_wave(x, win, out=y, dry_gain=g)
    torch.cuda.synchronize()
    kern = {k: {"avg_ms": v[0], "launches": v[1]} for k, v in eng.timing_read().items()}
    eng.timing_enable(False)
    return {"B": B, "seconds": seconds, "frames": 1 + L // 256, "k_istft_ms": kern["k_istft"]["avg_ms"],
            "k_istft_mix_ms": kern["k_istft_mix"]["avg_ms"],
            "ratio": kern["k_istft_mix"]["avg_ms"] / kern["k_istft"]["avg_ms"], "kernels_event_timed": kern}


def latency_n1(eng, win, iters):
    eng.reserve(1, 1)
    x = torch.randn(1, 256, device="cuda") * 0.1
    y = torch.empty_like(x)
    st = eng.new_wave_state(1, win)
    step = lambda: eng.wave_stream_step(st, x, out=y)             # noqa: E731
    timed(step, 50)
    eager = [timed(step, iters) for _ in range(5)]
    # host-side: the wall time of one call that ends in a synchronise
    walls = []
    for _ in range(200):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    warm = eng.new_wave_state(1, win)
    with torch.cuda.stream(s):
        eng.wave_stream_step(warm, x, out=y)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            eng.wave_stream_step(st, x, out=y)
    torch.cuda.synchronize()
    timed(g.replay, 50)
    graph = [timed(g.replay, iters) for _ in range(5)]
    return {"eager_device_ms_per_call": statistics.median(eager), "eager_wall_ms_per_call_synced": statistics.median(walls),
            "graph_replay_ms_per_call": statistics.median(graph), "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,1024,16384,65536")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wave_stream_bench.json"))
    ap.add_argument("--trace-only", type=int, default=0)
    ap.add_argument("--rate", action="store_true", help="the rate step at 48 / 8 kHz against the 16 kHz wave step")
    ap.add_argument("--highband", action="store_true",
                    help="with --rate: the plain 48 kHz rate step against the step with the high band, alternating; with "
                         "--packet: one period of the plain packet call against the call with the high band, 48 kHz / 480, 960")
    ap.add_argument("--trace-fs", type=int, default=48000)
    ap.add_argument("--packet", action="store_true",
                    help="the packet form at 16 kHz / 160, 320, 48 kHz / 480 and 44.1 kHz / 441 against the wave and rate steps")
    ap.add_argument("--trace-packet", type=int, default=480, help="--packet --trace-only: the packet, in samples at --trace-fs")
    ap.add_argument("--dry-gain", action="store_true",
                    help="the attenuation limit: plain against limited wave step, packet period (16 kHz / 160) and k_istft")
    ap.add_argument("--meters", action="store_true",
                    help="the level meters: plain against metered wave step and packet period (16 kHz / 160)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wave_stream_bench needs the GPU (nothing is measured on the CPU)")
    from gtcrn_micro_amd import Engine
    params = np.fromfile(os.path.join(ROOT, "tests", "golden", "params_dns3.f32"), dtype=np.float32)
    eng = Engine(params, 0)
    win = torch.hann_window(512).pow(0.5).cuda()
    if a.meters:
        sizes = [int(s) for s in a.sizes.split(",")] if a.sizes != ap.get_default("sizes") else [16384, 65536]
        out = a.out if "wave_stream_bench" not in a.out else os.path.join(ROOT, "profiles", "meters_bench.json")
        res = {"device": torch.cuda.get_device_name(0), "compare": []}
        for N in sizes:
            r = compare_meters(eng, win, N, a.iters, a.reps)
            print(json.dumps({k: v for k, v in r.items() if "reps" not in k and k != "kernels_event_timed"}), flush=True)
            res["compare"].append(r)
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", out)
        return
    if a.dry_gain:
        sizes = [int(s) for s in a.sizes.split(",")] if a.sizes != ap.get_default("sizes") else [16384, 65536]
        if a.trace_only:
            N = a.trace_only
            eng.reserve(N, 1)
            sp, sl = eng.new_wave_state(N, win), eng.new_wave_state(N, win, atten_lim_db=12)
            x = torch.randn(N, 256, device="cuda") * 0.1
            y = torch.empty_like(x)
            for _ in range(a.iters):
                eng.wave_stream_step(sp, x, out=y)
                eng.wave_stream_step(sl, x, out=y)
            torch.cuda.synchronize()
            del sp, sl
            torch.cuda.empty_cache()
            offline_dry_gain(eng, win, reps=5)
            return
        out = a.out if "wave_stream_bench" not in a.out else os.path.join(ROOT, "profiles", "dry_gain_bench.json")
        res = {"device": torch.cuda.get_device_name(0), "compare": []}
        for N in sizes:
            r = compare_dry_gain(eng, win, N, a.iters, a.reps)
            print(json.dumps({k: v for k, v in r.items() if "reps" not in k and k != "kernels_event_timed"}), flush=True)
            res["compare"].append(r)
        res["offline"] = offline_dry_gain(eng, win, reps=a.reps)
        print(json.dumps({k: v for k, v in res["offline"].items() if k != "kernels_event_timed"}), flush=True)
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", out)
        return
    if a.packet and a.highband:
        if a.trace_only:
            raise SystemExit("--packet --highband goes without --trace-only")
        sizes = [int(s) for s in a.sizes.split(",")] if a.sizes != ap.get_default("sizes") else [16384, 65536]
        out = a.out if "wave_stream_bench" not in a.out else os.path.join(ROOT, "profiles", "highband_packet_bench.json")
        res = {"device": torch.cuda.get_device_name(0), "compare": []}
        for N in sizes:
            r = compare_packet_highband(eng, win, N, a.iters, a.reps)
            for c in r["cases"]:
                print(json.dumps({"N": N, **{k: v for k, v in c.items() if "reps" not in k and k != "kernels_one_period"}}),
                      flush=True)
            res["compare"].append(r)
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", out)
        return
    if a.packet:
        sizes = [int(s) for s in a.sizes.split(",")] if a.sizes != ap.get_default("sizes") else [16384, 65536]
        if a.trace_only:
            st = eng.new_packet_state(a.trace_only, win, a.trace_packet, a.trace_fs)
            x = torch.randn(a.trace_only, a.trace_packet, device="cuda") * 0.1
            y = torch.empty_like(x)
            for _ in range(a.iters * st.period):
                eng.packet_stream_step(st, x, out=y)
            torch.cuda.synchronize()
            return
        out = a.out if "wave_stream_bench" not in a.out else os.path.join(ROOT, "profiles", "packet_stream_bench.json")
        res = {"device": torch.cuda.get_device_name(0), "compare": []}
        for N in sizes:
            r = compare_packet(eng, win, N, a.iters, a.reps)
            for c in r["cases"]:
                print(json.dumps({"N": N, **{k: v for k, v in c.items() if "reps" not in k and k != "kernels_one_period"}}),
                      flush=True)
            res["compare"].append(r)
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", out)
        return
    if a.highband:
        if not a.rate or a.trace_only:
            raise SystemExit("--highband goes with --rate (and without --trace-only)")
        sizes = [int(s) for s in a.sizes.split(",")] if a.sizes != ap.get_default("sizes") else [16384, 65536]
        out = a.out if "wave_stream_bench" not in a.out else os.path.join(ROOT, "profiles", "highband_rate_bench.json")
        res = {"device": torch.cuda.get_device_name(0), "compare": []}
        for N in sizes:
            r = compare_highband(eng, win, N, a.iters, a.reps)
            print(json.dumps({k: v for k, v in r.items() if "reps" not in k}), flush=True)
            res["compare"].append(r)
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", out)
        return
    if a.trace_only and a.rate:
        N = a.trace_only
        st = eng.new_rate_state(N, win, a.trace_fs)
        eng.rate_stream_reserve(st, 1)
        x = torch.randn(N, st.hop, device="cuda") * 0.1
        y = torch.empty_like(x)
        for _ in range(a.iters):
            eng.rate_stream_step(st, x, out=y)
        torch.cuda.synchronize()
        return
    if a.rate:
        out = a.out if "wave_stream_bench" not in a.out else os.path.join(ROOT, "profiles", "rate_stream_bench.json")
        res = {"device": torch.cuda.get_device_name(0), "compare": []}
        for N in [int(s) for s in a.sizes.split(",")]:
            r = compare_rate(eng, win, N, a.iters, a.reps)
            print(json.dumps({k: v for k, v in r.items() if "reps" not in k}), flush=True)
            res["compare"].append(r)
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", out)
        return
    if a.trace_only:
        N = a.trace_only
        eng.reserve(N, 1)
        st = eng.new_wave_state(N, win)
        x = torch.randn(N, 256, device="cuda") * 0.1
        y = torch.empty_like(x)
        for _ in range(a.iters):
            eng.wave_stream_step(st, x, out=y)
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "traffic": traffic_per_stream_step(4),
           "traffic_pcm16": traffic_per_stream_step(2)["total_bytes"], "compare": [], "latency_n1": None}
    for N in [int(s) for s in a.sizes.split(",")]:
        r = compare(eng, win, N, a.iters, a.reps)
        print(json.dumps({k: v for k, v in r.items() if not k.endswith("reps_ms")}), flush=True)
        res["compare"].append(r)
    res["latency_n1"] = latency_n1(eng, win, 500)
    print(json.dumps(res["latency_n1"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
