"""gtcrn_score_ext on the MI355X against the float64 checker (tests/score_ext_checker.py) and against gtcrn_score.

Tolerances.  profiles/score_ext_parity.json holds max |gpu - checker| of ESTOI and of segmental SNR (dB), measured by
measure() below over this file's checker comparisons on an MI355X (tools/score_ext_parity.py writes it); each tolerance
is 4 x that figure (box-to-box and compiler differences), the rule tests/test_gpu_score.py applies to STOI.  Both have a
ceiling that no measurement may move: 5e-5, half a unit of the %.4f RESULTS.txt prints.  SDR, SI-SNR and STOI are not
measured again here: bytes 0 .. 31 of a record are compared with gtcrn_score's bit for bit.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import score_checker as SC
import score_ext_checker as SX
from test_gpu_score import _make_folder, bits, to_batch

pytestmark = pytest.mark.gpu

PARITY_JSON = os.path.join(ROOT, "profiles", "score_ext_parity.json")
PARITY_CASES = ("L16000_B5", "L16000_B3", "var", "L64000_B1")
QUANTITIES = ("estoi", "segsnr_db")
CEILING = {"estoi": 5e-5, "segsnr_db": 5e-5}
ALL = ("sdr", "sisnr", "stoi", "estoi", "segsnr")


def tolerances():
    measured = json.load(open(PARITY_JSON))["measured"]
    tol = {}
    for q in QUANTITIES:
        assert float(measured[q]) <= CEILING[q], f"measured {q} error {measured[q]:.3e} exceeds {CEILING[q]:g}: a finding, not a tolerance"
        tol[q] = min(4.0 * float(measured[q]), CEILING[q])
    return tol


@pytest.fixture(scope="module")
def scorer():
    import torch
    assert torch.cuda.is_available()
    from gtcrn_micro_amd import Scorer
    sc = Scorer(0)
    yield sc
    sc.close()


def host(res):
    """A score_ext result on the host: the (B,8) records, and the int32 fields as columns."""
    return dict(rec=res["records"].cpu().numpy().copy(), kept=res["kept_frames"].cpu().numpy().copy(),
                segs=res["segments"].cpu().numpy().copy(), frames=res["segsnr_frames"].cpu().numpy().copy())


_cache = {}


def gpu_case(sc, name):
    if name not in _cache:
        L, specs = SC.GPU_CASES[name]
        ref, inf, lens = to_batch([SC.case_pair(sp) for sp in specs], L)
        _cache[name] = dict(host(sc.score_ext(ref, inf, lengths=lens)), specs=specs)
    return _cache[name]


def frames_to_length(nfr):
    """The shortest 16 kHz clip with nfr analysis frames at 10 kHz."""
    L = 8 * (256 + 128 * (nfr - 1)) // 5
    while SC.frames(L) < nfr:
        L += 1
    assert SC.frames(L) == nfr
    return L


def segment_edge_case(sc):
    """White-noise pairs (every frame kept) with M = 29, 30, 31 and 30 + (segments per workgroup) - 1, + 0, + 1."""
    if "segment_edges" not in _cache:
        from gtcrn_micro_amd._lib import SCORE_EXT_SEGS_PER_WG as G
        Ms = (29, 30, 31, 30 + G - 1, 30 + G, 30 + G + 1)
        rng = np.random.default_rng(20260)
        pairs = []
        for M in Ms:
            n = frames_to_length(M + 1)
            r = (0.1 * rng.standard_normal(n)).astype(np.float32)
            pairs.append((r, (r + 0.05 * rng.standard_normal(n)).astype(np.float32)))
        ref, inf, lens = to_batch(pairs, max(len(r) for r, _ in pairs))
        _cache["segment_edges"] = dict(host(sc.score_ext(ref, inf, lengths=lens)), pairs=pairs, Ms=Ms,
                                       want=[SX.score_ext(r, y) for r, y in pairs])
    return _cache["segment_edges"]


def frame_edge_case(sc):
    """n = 480 + 120 k + {-1, 0, 1} for k = 0 .. 40, and 0, 1, 479: every frame count from 0 to 41 at its edges."""
    if "frame_edges" not in _cache:
        ns = [0, 1, 479] + [480 + 120 * k + d for k in range(41) for d in (-1, 0, 1)]
        assert max(ns) < 5400
        rng = np.random.default_rng(20261)
        pairs = []
        for n in ns:
            r = (0.1 * rng.standard_normal(n)).astype(np.float32)
            pairs.append((r, (r + 0.03 * rng.standard_normal(n)).astype(np.float32)))
        ref, inf, lens = to_batch(pairs, max(ns))
        _cache["frame_edges"] = dict(host(sc.score_ext(ref, inf, lengths=lens, what=("segsnr",))), pairs=pairs, ns=ns,
                                     want=[SX.segsnr(r, y) for r, y in pairs])
    return _cache["frame_edges"]


def identical_case(sc):
    if "identical" not in _cache:
        r = SC.excerpt_pair(SC.examples(), 0, 8)[0]
        ref, inf, _ = to_batch([(r, r)], SC.EXCERPT_LEN)
        _cache["identical"] = dict(host(sc.score_ext(ref, inf)), pairs=[(r, r)])
    return _cache["identical"]


def silence_case(sc):
    if "silence" not in _cache:
        x = SC.excerpt_pair(SC.examples(), 1, 8, 16000)[0]
        z = np.zeros(16000, np.float32)
        pairs = [(z, x), (x, z), (z, z)]
        ref, inf, _ = to_batch(pairs, 16000)
        _cache["silence"] = dict(host(sc.score_ext(ref, inf)), pairs=pairs)
    return _cache["silence"]


def measure(sc, verbose=True):
    """max |gpu - checker| of ESTOI and of segmental SNR over every checker comparison of this file: the clips of
    PARITY_CASES, the segment-edge and frame-edge batches, a signal against itself and the silent pairs."""
    worst = {q: 0.0 for q in QUANTITIES}

    def note(tag, e):
        if verbose:
            print(tag, " ".join(f"{q} {v:.3e}" for q, v in e.items()))
        for q, v in e.items():
            worst[q] = max(worst[q], float(v))

    for name in PARITY_CASES:
        g = gpu_case(sc, name)
        for b, sp in enumerate(g["specs"]):
            want = SX.case_reference(sp)
            e = {"estoi": abs(g["rec"][b, 4] - want["estoi"])}
            if want["segsnr_frames"]:
                e["segsnr_db"] = abs(g["rec"][b, 5] - want["segsnr"])
            note(f"{name} {b} {sp}", e)
    g = segment_edge_case(sc)
    for b, want in enumerate(g["want"]):
        note(f"segment_edges M={g['Ms'][b]}", {"estoi": abs(g["rec"][b, 4] - want["estoi"]),
                                               "segsnr_db": abs(g["rec"][b, 5] - want["segsnr"])})
    g = frame_edge_case(sc)
    note("frame_edges", {"segsnr_db": max(abs(g["rec"][b, 5] - v) for b, (v, F) in enumerate(g["want"]) if F)})
    for name, g in (("identical", identical_case(sc)), ("silence", silence_case(sc))):
        for b, (r, y) in enumerate(g["pairs"]):
            want = SX.score_ext(r, y)
            note(f"{name} {b}", {"estoi": abs(g["rec"][b, 4] - want["estoi"]), "segsnr_db": abs(g["rec"][b, 5] - want["segsnr"])})
    return worst


def test_parity_with_the_checker(scorer):
    tol = tolerances()
    for name in PARITY_CASES:
        g = gpu_case(scorer, name)
        for b, sp in enumerate(g["specs"]):
            want = SX.case_reference(sp)
            assert want["stages"]["margin_db"] > SC.MASK_MARGIN_DB
            assert (g["kept"][b], g["segs"][b], g["frames"][b]) == (want["kept_frames"], want["segments"], want["segsnr_frames"]), (name, b)
            print(name, b, sp, f"estoi {g['rec'][b, 4]:.9f} ({want['estoi']:.9f}) segsnr {g['rec'][b, 5]:.9f} ({want['segsnr']:.9f})")
            assert abs(g["rec"][b, 4] - want["estoi"]) <= tol["estoi"], (name, b)
            if want["segsnr_frames"]:
                assert abs(g["rec"][b, 5] - want["segsnr"]) <= tol["segsnr_db"], (name, b)
            else:
                assert np.isnan(g["rec"][b, 5])
            assert np.all(g["rec"][b, 6:].view(np.int32)[1:] == 0)
    var = gpu_case(scorer, "var")                          # 6000 and 257 samples: no segment; 257: no frame either
    assert var["rec"][2, 4] == 1e-5 and var["rec"][4, 4] == 1e-5 and var["frames"][2] == 47 and var["frames"][4] == 0


def test_segment_edges(scorer):
    tol = tolerances()
    g = segment_edge_case(scorer)
    for b, want in enumerate(g["want"]):
        st = want["stages"]
        M = g["Ms"][b]
        assert st["kept_frames"] == st["n"] == M + 1 and st["margin_db"] >= SC.MASK_MARGIN_DB      # every frame is kept
        assert want["segments"] == max(M - 29, 0)
        assert (g["kept"][b], g["segs"][b]) == (M + 1, max(M - 29, 0)), M
        print("M", M, "estoi", g["rec"][b, 4], want["estoi"])
        assert abs(g["rec"][b, 4] - want["estoi"]) <= tol["estoi"], M
        assert abs(g["rec"][b, 5] - want["segsnr"]) <= tol["segsnr_db"], M
    assert g["rec"][0, 4] == 1e-5 and 0.0 < g["rec"][1, 4] < 1.0


def test_frame_edges(scorer):
    tol = tolerances()
    g = frame_edge_case(scorer)
    for b, (v, F) in enumerate(g["want"]):
        n = g["ns"][b]
        assert F == SX.segsnr_frames(n) and g["frames"][b] == F, n
        if F == 0:
            assert np.isnan(g["rec"][b, 5]), n
        else:
            assert abs(g["rec"][b, 5] - v) <= tol["segsnr_db"], (n, g["rec"][b, 5], v)
    assert sorted(set(F for _, F in g["want"])) == list(range(42))
    assert np.all(g["rec"].view(np.int64)[:, :5] == 0)                    # only segmental SNR was asked for


def test_up_to_seven_is_gtcrn_score_with_zeros_behind(scorer):
    L, specs = SC.GPU_CASES["var"]
    ref, inf, lens = to_batch([SC.case_pair(sp) for sp in specs], L)
    names = ("sdr", "sisnr", "stoi")
    for mask in range(1, 8):
        what = tuple(n for i, n in enumerate(names) if mask >> i & 1)
        old = bits(scorer.score(ref, inf, lengths=lens, what=what)["records"])
        new = bits(scorer.score_ext(ref, inf, lengths=lens, what=what)["records"])
        assert np.array_equal(new[:, :4], old), what
        assert np.all(new[:, 4:] == 0), what


def test_what_masks_zero_the_rest_and_keep_the_bits(scorer):
    L, specs = SC.GPU_CASES["L16000_B3"]
    ref, inf, _ = to_batch([SC.case_pair(sp) for sp in specs], L)
    full = bits(scorer.score_ext(ref, inf)["records"])
    assert np.all(full[:, :6] != 0) and np.all(full[:, 7] == 0)
    col = {"sdr": 0, "sisnr": 1, "stoi": 2, "estoi": 4, "segsnr": 5}
    for mask in range(1, 32):
        what = tuple(n for i, n in enumerate(ALL) if mask >> i & 1)
        got = bits(scorer.score_ext(ref, inf, what=what)["records"])
        for n, c in col.items():
            assert np.array_equal(got[:, c], full[:, c] if n in what else np.zeros_like(got[:, c])), (what, n)
        assert np.array_equal(got[:, 3], full[:, 3] if mask & 12 else np.zeros_like(got[:, 3])), what      # kept_frames, segments
        assert np.array_equal(got[:, 6], full[:, 6] if mask & 16 else np.zeros_like(got[:, 6])), what      # segsnr_frames
        assert np.all(got[:, 7] == 0)


def test_a_record_does_not_depend_on_batch_row_padding_or_neighbours(scorer):
    specs = SC.GPU_CASES["var"][1]
    a = SC.case_pair(specs[3])                              # 40001 samples
    others = [SC.case_pair(sp) for sp in (specs[0], specs[1], specs[2], specs[4])]   # 64000, 16000, 6000, 257
    alone = bits(scorer.score_ext(*to_batch([a], 40001)[:2])["records"])[0]
    assert SX.case_reference(specs[3])["segments"] > 0 and alone[4] != 0 and alone[5] != 0
    for row in (0, 2, 4):
        batch = list(others)
        batch.insert(row, a)
        ref, inf, lens = to_batch(batch, 64000)             # (NaN behind every length)
        got = bits(scorer.score_ext(ref, inf, lengths=lens)["records"])[row]
        assert np.array_equal(got, alone), row
    for batch in ([others[2], a, others[3]], [others[0], a]):
        ref, inf, lens = to_batch(batch, 64000 if len(batch) == 2 else 40001)
        got = bits(scorer.score_ext(ref, inf, lengths=lens)["records"])[1]
        assert np.array_equal(got, alone)


def test_a_nan_or_inf_in_one_clip_changes_no_bit_of_another(scorer):
    import torch
    L, specs = SC.GPU_CASES["L16000_B3"]
    ref, inf, _ = to_batch([SC.case_pair(sp) for sp in specs], L)
    clean = bits(scorer.score_ext(ref, inf)["records"])
    for bad in (float("nan"), float("inf"), float("-inf")):
        for victim in ("ref", "inf"):
            r2, y2 = ref.clone(), inf.clone()
            (r2 if victim == "ref" else y2)[1, 5003] = bad
            res = scorer.score_ext(r2, y2)
            torch.cuda.synchronize()
            got = bits(res["records"])
            assert np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2]), (bad, victim)
            k, s = int(res["kept_frames"][1]), int(res["segments"][1])
            assert 0 <= k <= SC.frames(L) and 0 <= s <= max(k - 30, 0), (k, s)
            assert int(res["segsnr_frames"][1]) == SX.segsnr_frames(L)
            e = float(res["estoi"][1])
            assert e != e or e == 1e-5 or -1.0 <= e <= 1.0
        again = bits(scorer.score_ext(ref, inf)["records"])
        assert np.array_equal(again, clean), bad


def test_silence_and_identity_give_what_the_formulas_give(scorer):
    tol = tolerances()
    g = silence_case(scorer)
    rec = g["rec"]
    assert np.isfinite(rec[:, :6]).all()
    assert np.all(rec[:, 4] == 0.0)                                  # ESTOI: exactly 0 when either signal is all zero
    assert rec[0, 5] == -10.0 and rec[2, 5] == -10.0 and abs(rec[1, 5]) <= 1e-6
    for b, (r, y) in enumerate(g["pairs"]):
        want = SX.score_ext(r, y)
        assert (g["kept"][b], g["segs"][b], g["frames"][b]) == (want["kept_frames"], want["segments"], want["segsnr_frames"])
        assert abs(rec[b, 5] - want["segsnr"]) <= tol["segsnr_db"]
    rec = identical_case(scorer)["rec"][0]
    print("x against x: ESTOI", repr(rec[4]), "segsnr", rec[5])
    assert rec[5] == 35.0 and abs(rec[4] - 1.0) <= tol["estoi"]


def test_strided_and_broadcast_rows(scorer):
    import torch
    L, specs = SC.GPU_CASES["L16000_B3"]
    ref, inf, _ = to_batch([SC.case_pair(sp) for sp in specs], L)
    want = bits(scorer.score_ext(ref, inf)["records"])
    wide_r = torch.full((3, L + 37), float("nan"), device="cuda")
    wide_y = torch.full((3, L + 5), float("nan"), device="cuda")
    wide_r[:, :L] = ref
    wide_y[:, :L] = inf
    assert np.array_equal(bits(scorer.score_ext(wide_r[:, :L], wide_y[:, :L])["records"]), want)
    one = bits(scorer.score_ext(ref[0:1].repeat(3, 1), inf)["records"])
    got = bits(scorer.score_ext(ref[0:1].expand(3, L), inf)["records"])
    assert np.array_equal(got, one) and np.array_equal(one[0], want[0]) and not np.array_equal(one[1], want[1])


def test_bad_arguments_are_refused_before_any_launch(scorer):
    import torch
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd._lib import lib
    x = torch.zeros((2, 4000), device="cuda")
    out = torch.full((2, 8), 7.0, device="cuda", dtype=torch.float64)
    ws = torch.zeros(scorer.ext_workspace_bytes(2, 4000), device="cuda", dtype=torch.uint8)
    ok = [scorer._h, x.data_ptr(), 4000, x.data_ptr(), 4000, None, 4000, 2, 31, out.data_ptr(), ws.data_ptr(), None]
    for pos, val in ((1, None), (3, None), (9, None), (10, None), (2, 3999), (4, 3999), (6, 0), (7, 0), (8, 0), (8, 32),
                     (8, -1), (10, ws.data_ptr() + 4), (9, out.data_ptr() + 4)):
        args = list(ok)
        args[pos] = val
        assert lib().gtcrn_score_ext(*args) == -1, (pos, val)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                   # nothing was launched
    for what in (8, 16, 4):                                           # each of the three needs the workspace
        args = list(ok)
        args[8], args[10] = what, None
        assert lib().gtcrn_score_ext(*args) == -1, what
    args = list(ok)
    args[8], args[10] = 3, None                                       # SDR and SI-SNR do not
    assert lib().gtcrn_score_ext(*args) == 0
    assert lib().gtcrn_score_ext(*ok) == 0
    torch.cuda.synchronize()
    with pytest.raises(GtcrnError):
        scorer.score_ext(x, x[:, :100])
    with pytest.raises(GtcrnError):
        scorer.score_ext(x, x, what=("pesq",))
    with pytest.raises(GtcrnError):
        scorer.score_ext(x, x, out=torch.zeros((2, 4), device="cuda", dtype=torch.float64))


def test_the_call_is_captured_in_a_graph_and_replayed_on_new_data(scorer):
    import torch
    L, specs = SC.GPU_CASES["L16000_B3"]
    a = to_batch([SC.case_pair(sp) for sp in specs], L)
    b = to_batch([SC.case_pair(sp) for sp in SC.GPU_CASES["L16000_B5"][1][:3]], L)
    want_a, want_b = bits(scorer.score_ext(a[0], a[1])["records"]), bits(scorer.score_ext(b[0], b[1])["records"])
    ref, inf = a[0].clone(), a[1].clone()
    out = torch.zeros((3, 8), device="cuda", dtype=torch.float64)
    scorer.score_ext(ref, inf, out=out)                 # (the workspace for this shape exists before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scorer.score_ext(ref, inf, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(out), want_a)
    ref.copy_(b[0])
    inf.copy_(b[1])
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(out), want_b) and not np.array_equal(want_a, want_b)


def test_score_batch_routes_the_new_names_to_score_ext(scorer):
    from gtcrn_micro_amd.train import score_batch
    L, specs = SC.GPU_CASES["L16000_B3"]
    ref, inf, _ = to_batch([SC.case_pair(sp) for sp in specs], L)
    for what in (("sdr", "estoi", "segsnr"), ALL, ("segsnr",)):
        res = score_batch(ref, inf, scorer, what=what)
        assert tuple(res["records"].shape) == (3, 8) and "estoi" in res and "segsnr_frames" in res
        assert np.array_equal(bits(res["records"]), bits(scorer.score_ext(ref, inf, what=what)["records"])), what
    old = score_batch(ref, inf, scorer, what=("sdr", "stoi"))               # the present path, with the same bits
    assert tuple(old["records"].shape) == (3, 4) and "estoi" not in old
    assert np.array_equal(bits(old["records"]), bits(scorer.score(ref, inf, what=("sdr", "stoi"))["records"]))


def test_folder_driver_writes_the_two_extra_files_only_with_the_flag(tmp_path, scorer):
    import torch
    from gtcrn_micro_amd.infer import enhance_folder, read_wav_f32
    noisy_dir, clean_dir, n16 = _make_folder(tmp_path)
    ck = os.path.join(GOLDEN, "params_dns3.f32")
    scored, ext = tmp_path / "enh_scored", tmp_path / "enh_ext"
    inf_scp, _ = enhance_folder(str(noisy_dir), str(clean_dir), str(scored), ck, max_batch=3, score=True)
    enhance_folder(str(noisy_dir), str(clean_dir), str(ext), ck, max_batch=3, score_ext=True)      # (implies score)
    wavs = sorted(uid + "_enh.wav" for uid, _ in inf_scp)
    old = ["SDR.scp", "SISNR.scp", "STOI.scp", "RESULTS.txt"]
    assert sorted(os.listdir(scored)) == sorted(wavs + ["inf.scp", "ref.scp"] + old)
    assert sorted(os.listdir(ext)) == sorted(wavs + ["inf.scp", "ref.scp"] + old + ["ESTOI.scp", "SSNR.scp"])
    for name in wavs + old[:3]:
        assert open(scored / name, "rb").read() == open(ext / name, "rb").read(), name
    table = {m: dict(ln.split() for ln in open(ext / f"{m}.scp")) for m in ("ESTOI", "SSNR")}
    uids = [uid for uid, _ in inf_scp if not uid.endswith("_90")]
    assert len(uids) == n16 and all(list(t) == uids for t in table.values())      # the order of inf.scp
    means = {m: [] for m in table}
    for uid in uids:
        _, enh = read_wav_f32(str(ext / f"{uid}_enh.wav"))
        _, clean = read_wav_f32(str(clean_dir / f"clean_fileid_{uid.split('fileid_')[-1]}.wav"))
        res = scorer.score_ext(torch.from_numpy(clean).cuda(), torch.from_numpy(enh).cuda())
        for m, key in (("ESTOI", "estoi"), ("SSNR", "segsnr")):
            assert table[m][uid] == repr(float(res[key][0])), (uid, m)
            means[m].append(float(res[key][0]))
    plain, lines = open(scored / "RESULTS.txt").read().splitlines(), open(ext / "RESULTS.txt").read().splitlines()
    assert lines[:3] == plain[:3] and lines[5:] == plain[3:]
    assert lines[3:5] == [f"{m}: {np.nanmean(means[m]):.4f}" for m in ("ESTOI", "SSNR")]
