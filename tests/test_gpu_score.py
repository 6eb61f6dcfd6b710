"""gtcrn_score on the MI355X against the float64 checker (tests/score_checker.py) and the reference's own numbers.

Tolerances.  profiles/score_parity.json holds max |gpu - checker| per quantity, measured by measure() below over exactly
this file's inputs on an MI355X (tools/score_parity.py writes it); each tolerance is 4 x that (box-to-box and compiler
differences).  For the three scores there is a ceiling that no measurement may move: 5e-5 (half a unit of the %.4f
RESULTS.txt prints) for STOI, 5e-5 dB for SDR and SI-SNR.  STOI of the synthetic_mix clips of the score_batch test is
measured under a key of its own (stoi_synthetic_mix): their reference has empty third-octave bands, see that test.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import score_checker as SC

pytestmark = pytest.mark.gpu

PARITY_JSON = os.path.join(ROOT, "profiles", "score_parity.json")
QUANTITIES = ("x10", "energies_db", "env", "sdr_db", "sisnr_db", "stoi")
SYNTH = "stoi_synthetic_mix"
CEILING = {"sdr_db": 5e-5, "sisnr_db": 5e-5, "stoi": 5e-5, SYNTH: 5e-5}

def tolerances():
    measured = json.load(open(PARITY_JSON))["measured"]
    tol = {q: 4.0 * float(measured[q]) for q in QUANTITIES + (SYNTH,)}
    for q, c in CEILING.items():
        assert float(measured[q]) <= c, f"measured {q} error {measured[q]:.3e} exceeds {c:g}: a finding, not a tolerance"
        tol[q] = min(tol[q], c)
    return tol


@pytest.fixture(scope="module")
def scorer():
    import torch
    assert torch.cuda.is_available()
    from gtcrn_micro_amd import Scorer
    sc = Scorer(0)
    yield sc
    sc.close()


def to_batch(pairs, L):
    """(ref, inf, lengths or None): rows padded with NaN behind their length -- nothing may read there."""
    import torch
    ref = np.full((len(pairs), L), np.nan, np.float32)
    inf = np.full((len(pairs), L), np.nan, np.float32)
    for b, (r, y) in enumerate(pairs):
        ref[b, :len(r)] = r
        inf[b, :len(y)] = y
    lens = [len(r) for r, _ in pairs]
    return torch.from_numpy(ref).cuda(), torch.from_numpy(inf).cuda(), (None if min(lens) == L else lens)


def bits(rec):
    """(B,4) float64 records -> their 32 bytes per row as int64, on the host."""
    import torch
    return rec.contiguous().view(torch.int64).cpu().numpy().copy()


_case_cache = {}


def gpu_case(sc, name):
    """One batch of SC.GPU_CASES through the scorer, with every debug hook read back; computed once."""
    if name not in _case_cache:
        L, specs = SC.GPU_CASES[name]
        ref, inf, lens = to_batch([SC.case_pair(sp) for sp in specs], L)
        res = sc.score(ref, inf, lengths=lens)
        rec = res["records"].cpu().numpy().copy()
        counts = np.stack([res["kept_frames"].cpu().numpy(), res["segments"].cpu().numpy()], 1)
        hooks = [[sc.debug(w, b).cpu().numpy() for w in range(5)] for b in range(len(specs))]
        _case_cache[name] = dict(rec=rec, counts=counts, hooks=hooks, specs=specs)
    return _case_cache[name]


def peak_rel(got, want):
    if want.size == 0:
        assert got.size == 0
        return 0.0
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got.astype(np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


def measure(sc, verbose=True):
    """max |gpu - checker| per quantity over every clip of SC.GPU_CASES (x10 and env relative to the clip's peak)."""
    worst = {q: 0.0 for q in QUANTITIES}
    for name in SC.GPU_CASES:
        g = gpu_case(sc, name)
        for b, sp in enumerate(g["specs"]):
            want = SC.case_reference(sp)
            st = want["stages"]
            h = g["hooks"][b]
            e = {"x10": peak_rel(h[0], st["x10"]),
                 "energies_db": float(np.abs(h[1] - st["energies"]).max()) if st["n"] else 0.0,
                 "env": max(peak_rel(h[3], st["env_ref"]), peak_rel(h[4], st["env_inf"])),
                 "sdr_db": abs(g["rec"][b, 0] - want["sdr"]), "sisnr_db": abs(g["rec"][b, 1] - want["sisnr"]),
                 "stoi": abs(g["rec"][b, 2] - want["stoi"])}
            if verbose:
                print(name, b, sp, " ".join(f"{q} {v:.3e}" for q, v in e.items()))
            for q in QUANTITIES:
                worst[q] = max(worst[q], float(e[q]))
    # the scores of the file's other inputs: a signal against itself, the silent pairs, the validate_batch output
    for name, (pairs, rec) in (("identical", identical_case(sc)), ("silence", silence_case(sc))):
        for b, (r, y) in enumerate(pairs):
            want = SC.score(r, y)
            e = {"sdr_db": abs(rec[b, 0] - want["sdr"]), "sisnr_db": abs(rec[b, 1] - want["sisnr"]),
                 "stoi": abs(rec[b, 2] - want["stoi"])}
            if verbose:
                print(name, b, " ".join(f"{q} {v:.3e}" for q, v in e.items()))
            for q in e:
                worst[q] = max(worst[q], float(e[q]))
    worst[SYNTH] = 0.0
    c, w, rec = surface_case(sc)[:3]
    for b in range(len(c)):
        want = SC.score(c[b], w[b])
        e = {"sdr_db": abs(rec[b, 0] - want["sdr"]), "sisnr_db": abs(rec[b, 1] - want["sisnr"]), SYNTH: abs(rec[b, 2] - want["stoi"])}
        if verbose:
            print("synthetic_mix", b, " ".join(f"{q} {v:.3e}" for q, v in e.items()))
        for q in e:
            worst[q] = max(worst[q], float(e[q]))
    return worst


_other = {}


def identical_case(sc):
    if "identical" not in _other:
        r = SC.excerpt_pair(SC.examples(), 0, 8)[0]
        ref, inf, _ = to_batch([(r, r)], SC.EXCERPT_LEN)
        _other["identical"] = ([(r, r)], sc.score(ref, inf)["records"].cpu().numpy().copy())
    return _other["identical"]


def silence_case(sc):
    if "silence" not in _other:
        x = SC.excerpt_pair(SC.examples(), 1, 8, 16000)[0]
        z = np.zeros(16000, np.float32)
        pairs = [(z, x), (x, z), (z, z)]
        ref, inf, _ = to_batch(pairs, 16000)
        _other["silence"] = (pairs, sc.score(ref, inf)["records"].cpu().numpy().copy())
    return _other["silence"]


def surface_case(sc):
    """(clean, enhanced, records, records of Scorer.score) of train.score_batch on a validate_batch output, on the host."""
    if "surface" not in _other:
        import torch
        from gtcrn_micro_amd.train import make_training, score_batch, synthetic_mix, validate_batch
        torch.manual_seed(7)
        model, _, _, loss_func = make_training(device="cuda")
        model.eval()
        noisy, clean = synthetic_mix(3, samples=16000, seed=9)
        _, wave = validate_batch(model, loss_func, noisy, clean)
        res = score_batch(clean, wave, sc)
        direct = sc.score(clean.contiguous(), wave.contiguous())
        _other["surface"] = (clean.cpu().numpy(), wave.cpu().numpy(), res["records"].cpu().numpy().copy(),
                             bits(res["records"]), bits(direct["records"]))
    return _other["surface"]


def test_parity_with_the_checker(scorer):
    tol = tolerances()
    for name in SC.GPU_CASES:
        g = gpu_case(scorer, name)
        for b, sp in enumerate(g["specs"]):
            want = SC.case_reference(sp)
            st = want["stages"]
            assert st["margin_db"] > SC.MASK_MARGIN_DB
            assert tuple(g["counts"][b]) == (want["kept_frames"], want["segments"]), (name, b)
            assert np.array_equal(g["hooks"][b][2] != 0, st["mask"]), (name, b)
            assert g["hooks"][b][0].size == st["x10"].size and g["hooks"][b][3].shape == (15, st["M"])
    worst = measure(scorer)
    print("worst:", worst, "tolerance:", tol)
    for q in QUANTITIES:
        assert worst[q] <= tol[q], f"{q}: {worst[q]:.3e} > {tol[q]:.3e}"


def test_short_rows_take_the_constant_path(scorer):
    g = gpu_case(scorer, "var")
    assert [sp[3] for sp in g["specs"]] == [64000, 16000, 6000, 40001, 257]
    assert g["rec"][2, 2] == 1e-5 and tuple(g["counts"][2]) == (28, 0)
    assert g["rec"][4, 2] == 1e-5 and tuple(g["counts"][4]) == (0, 0)
    assert g["hooks"][4][1].size == 0 and g["hooks"][4][0].size == 161
    assert np.isfinite(g["rec"]).all()


def test_sdr_and_sisnr_against_the_references_numbers(scorer):
    """The reference's own sdr_metric / sisnr_metric (float32 numpy) on the same float32 pairs, recorded in
    score_ref.npz: within the reference's noise floor (MANIFEST_score.json) plus this file's tolerance."""
    gold = np.load(os.path.join(GOLDEN, "score_ref.npz"))
    man = json.load(open(os.path.join(GOLDEN, "MANIFEST_score.json")))
    tol = tolerances()
    ex = SC.examples()
    pairs = [SC.excerpt_pair(ex, c, o) for c, o in SC.EXCERPTS] + [SC.ladder_pair(ex, s) for s in SC.SNR_LADDER]
    got = []
    for k in range(0, len(pairs), 5):
        ref, inf, _ = to_batch(pairs[k:k + 5], SC.EXCERPT_LEN)
        got.append(scorer.score(ref, inf, what=("sdr", "sisnr"))["records"].cpu().numpy())
    got = np.concatenate(got)
    d_sdr, d_sisnr = np.abs(got[:, 0] - gold["sdr"]).max(), np.abs(got[:, 1] - gold["sisnr"]).max()
    print(f"max |gpu - reference|: SDR {d_sdr:.3e} dB, SI-SNR {d_sisnr:.3e} dB")
    assert d_sdr <= man["sdr_reference_float32_vs_checker_float64_max_db"] + tol["sdr_db"]
    assert d_sisnr <= man["sisnr_reference_float32_vs_checker_float64_max_db"] + tol["sisnr_db"]
    assert np.all(got[:, 2:] == 0.0)


def test_identical_signals_give_what_the_formulas_give(scorer):
    tol = tolerances()
    (pair,), rec = identical_case(scorer)
    r, rec = pair[0], rec[0]
    want_sdr, want_sisnr = SC.sdr(r, r), SC.sisnr(r, r)
    print(f"x against x: SDR {rec[0]:.9f} (checker {want_sdr:.9f}), SI-SNR {rec[1]:.9f} ({want_sisnr:.9f}), STOI {rec[2]!r}")
    assert np.isfinite(rec[:3]).all() and 90.0 < want_sdr < 120.0      # the 1e-8 terms, not infinity
    assert abs(rec[0] - want_sdr) <= tol["sdr_db"] and abs(rec[1] - want_sisnr) <= tol["sisnr_db"]
    assert abs(rec[2] - 1.0) <= tol["stoi"]


def test_a_record_does_not_depend_on_batch_row_or_neighbours(scorer):
    specs = SC.GPU_CASES["var"][1]
    a = SC.case_pair(specs[3])                              # 40001 samples
    others = [SC.case_pair(sp) for sp in (specs[0], specs[1], specs[2], specs[4])]   # 64000, 16000, 6000, 257
    alone = bits(scorer.score(*to_batch([a], 40001)[:2])["records"])[0]
    assert SC.case_reference(specs[3])["segments"] > 0
    for row in (0, 2, 4):
        batch = list(others)
        batch.insert(row, a)
        ref, inf, lens = to_batch(batch, 64000)
        got = bits(scorer.score(ref, inf, lengths=lens)["records"])[row]
        assert np.array_equal(got, alone), row
    # next to shorter neighbours only, and to longer ones only, in a batch of another size
    for batch in ([others[2], a, others[3]], [others[0], a]):
        ref, inf, lens = to_batch(batch, 64000 if len(batch) == 2 else 40001)
        got = bits(scorer.score(ref, inf, lengths=lens)["records"])[1]
        assert np.array_equal(got, alone)


def test_a_nan_or_inf_in_one_clip_changes_no_bit_of_another(scorer):
    import torch
    L, specs = SC.GPU_CASES["L16000_B3"]
    ref, inf, _ = to_batch([SC.case_pair(sp) for sp in specs], L)
    clean = bits(scorer.score(ref, inf)["records"])
    for bad in (float("nan"), float("inf"), float("-inf")):
        for victim in ("ref", "inf"):
            r2, y2 = ref.clone(), inf.clone()
            (r2 if victim == "ref" else y2)[1, 5003] = bad
            res = scorer.score(r2, y2)
            torch.cuda.synchronize()
            got = bits(res["records"])
            assert np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2]), (bad, victim)
            k, s = int(res["kept_frames"][1]), int(res["segments"][1])
            assert 0 <= k <= SC.frames(L) and 0 <= s <= max(k - 30, 0), (k, s)
            stoi = float(res["stoi"][1])
            assert stoi != stoi or stoi == 1e-5 or -1.0 <= stoi <= 1.0
        again = bits(scorer.score(ref, inf)["records"])
        assert np.array_equal(again, clean), bad


def test_silence_keeps_every_score_defined(scorer):
    tol = tolerances()
    pairs, _ = silence_case(scorer)
    ref, inf, _ = to_batch(pairs, 16000)
    res = scorer.score(ref, inf)
    rec = res["records"].cpu().numpy()
    for b, (r, y) in enumerate(pairs):
        want = SC.score(r, y)
        print(b, rec[b, :3], (want["sdr"], want["sisnr"], want["stoi"]))
        assert np.isfinite(rec[b, :3]).all()
        assert int(res["kept_frames"][b]) == want["kept_frames"] and int(res["segments"][b]) == want["segments"]
        assert abs(rec[b, 0] - want["sdr"]) <= tol["sdr_db"] and abs(rec[b, 1] - want["sisnr"]) <= tol["sisnr_db"]
        assert abs(rec[b, 2] - want["stoi"]) <= tol["stoi"]


def test_what_masks_zero_the_rest_and_keep_the_bits(scorer):
    L, specs = SC.GPU_CASES["L16000_B3"]
    ref, inf, _ = to_batch([SC.case_pair(sp) for sp in specs], L)
    full = bits(scorer.score(ref, inf)["records"])
    names = ("sdr", "sisnr", "stoi")
    for mask in range(1, 7):
        what = tuple(n for i, n in enumerate(names) if mask >> i & 1)
        got = bits(scorer.score(ref, inf, what=what)["records"])
        for i in range(3):
            assert np.array_equal(got[:, i], full[:, i] if mask >> i & 1 else np.zeros_like(got[:, i])), (what, names[i])
        assert np.array_equal(got[:, 3], full[:, 3] if mask & 4 else np.zeros_like(got[:, 3])), what


def test_bad_arguments_are_refused_before_any_launch(scorer):
    import torch
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd._lib import lib
    x = torch.zeros((2, 4000), device="cuda")
    out = torch.zeros((2, 4), device="cuda", dtype=torch.float64)
    ws = torch.zeros(scorer.workspace_bytes(2, 4000), device="cuda", dtype=torch.uint8)
    ok = [scorer._h, x.data_ptr(), 4000, x.data_ptr(), 4000, None, 4000, 2, 7, out.data_ptr(), ws.data_ptr(), None]
    for pos, val in ((1, None), (3, None), (9, None), (10, None), (2, 3999), (4, 3999), (6, 0), (7, 0), (8, 0), (8, 8),
                     (10, ws.data_ptr() + 4)):
        args = list(ok)
        args[pos] = val
        assert lib().gtcrn_score(*args) == -1, (pos, val)
    assert lib().gtcrn_score(*ok) == 0
    torch.cuda.synchronize()
    with pytest.raises(GtcrnError):
        scorer.score(x, x[:, :100])
    with pytest.raises(GtcrnError):
        scorer.score(x, x, what=("pesq",))


def test_the_call_is_captured_in_a_graph_and_replayed_on_new_data(scorer):
    import torch
    L, specs = SC.GPU_CASES["L16000_B3"]
    a = to_batch([SC.case_pair(sp) for sp in specs], L)
    b = to_batch([SC.case_pair(sp) for sp in SC.GPU_CASES["L16000_B5"][1][:3]], L)
    want_a, want_b = bits(scorer.score(a[0], a[1])["records"]), bits(scorer.score(b[0], b[1])["records"])
    ref, inf = a[0].clone(), a[1].clone()
    out = torch.zeros((3, 4), device="cuda", dtype=torch.float64)
    scorer.score(ref, inf, out=out)                     # (the workspace for this shape exists before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scorer.score(ref, inf, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(out), want_a)
    ref.copy_(b[0])
    inf.copy_(b[1])
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(out), want_b) and not np.array_equal(want_a, want_b)


def test_score_batch_on_a_validate_batch_output(scorer):
    """train.score_batch is Scorer.score on the pair validate_batch hands back, to the bit.  Against the checker SDR and
    SI-SNR keep this file's tolerance.  STOI has a measurement of its own (stoi_synthetic_mix in score_parity.json, 4 x
    as everywhere, under the same 5e-5 ceiling): synthetic_mix's clean signal is five harmonics below 1.5 kHz, so most of
    its third-octave bands hold window leakage only, which the fp32 transform of steps 3-5 resolves to its rounding noise
    and float64 to the leakage itself; STOI normalises every band, so those bands count like the others."""
    c, w, rec, got_bits, direct_bits = surface_case(scorer)
    assert np.array_equal(got_bits, direct_bits)
    tol = tolerances()
    for b in range(3):
        want = SC.score(c[b], w[b])
        assert want["stages"]["margin_db"] > SC.MASK_MARGIN_DB, b      # (holds for this seed: the counts are compared exactly)
        print(b, "stoi", rec[b, 2], want["stoi"], abs(rec[b, 2] - want["stoi"]))
        assert abs(rec[b, 0] - want["sdr"]) <= tol["sdr_db"] and abs(rec[b, 1] - want["sisnr"]) <= tol["sisnr_db"]
        assert abs(rec[b, 2] - want["stoi"]) <= tol[SYNTH]
        assert tuple(rec[b, 3:].view(np.int32)) == (want["kept_frames"], want["segments"])


def test_a_broadcast_reference_is_scored_row_by_row(scorer):
    """One clean clip against B outputs: clean.expand(B, L) has stride 0 between its rows."""
    L, specs = SC.GPU_CASES["L16000_B3"]
    ref, inf, _ = to_batch([SC.case_pair(sp) for sp in specs], L)
    want = bits(scorer.score(ref[0:1].repeat(3, 1), inf)["records"])
    got = bits(scorer.score(ref[0:1].expand(3, L), inf)["records"])
    assert np.array_equal(got, want) and not np.array_equal(want[0], want[1])


def _make_folder(tmp_path, with_8k=True):
    from scipy.io import wavfile
    ex = SC.examples()
    noisy_dir, clean_dir = tmp_path / "noisy", tmp_path / "clean"
    noisy_dir.mkdir()
    clean_dir.mkdir()
    lengths = (16000, 17003, 20000, 24000, 24001, 30000, 31999, 12000)
    for k, n in enumerate(lengths):
        a = 16000 * (3 + 2 * k)
        wavfile.write(str(noisy_dir / f"mix_fileid_{k}.wav"), 16000, ex["noisy"][k % 5, a:a + n])
        wavfile.write(str(clean_dir / f"clean_fileid_{k}.wav"), 16000, ex["enh"][k % 5, a:a + n - 37 * (k % 3)])
    if with_8k:
        wavfile.write(str(noisy_dir / "mix_fileid_90.wav"), 8000, ex["noisy"][0, 0:16000:2].copy())
        wavfile.write(str(clean_dir / "clean_fileid_90.wav"), 16000, ex["enh"][0, 0:16000])
    return noisy_dir, clean_dir, len(lengths)


def test_folder_driver_scores_what_it_wrote_and_writes_nothing_else_without_the_flag(tmp_path, scorer):
    import torch
    from gtcrn_micro_amd.infer import enhance_folder, read_wav_f32
    noisy_dir, clean_dir, n16 = _make_folder(tmp_path)
    ck = os.path.join(GOLDEN, "params_dns3.f32")
    plain, scored, serial = tmp_path / "enh_plain", tmp_path / "enh_scored", tmp_path / "enh_serial"
    inf_scp, _ = enhance_folder(str(noisy_dir), str(clean_dir), str(plain), ck, max_batch=3)
    enhance_folder(str(noisy_dir), str(clean_dir), str(scored), ck, max_batch=3, score=True)
    enhance_folder(str(noisy_dir), str(clean_dir), str(serial), ck, max_batch=3, score=True, pipeline=False)
    wavs = sorted(uid + "_enh.wav" for uid, _ in inf_scp)
    assert sorted(os.listdir(plain)) == sorted(wavs + ["inf.scp", "ref.scp"])
    extra = ["SDR.scp", "SISNR.scp", "STOI.scp", "RESULTS.txt"]
    assert sorted(os.listdir(scored)) == sorted(wavs + ["inf.scp", "ref.scp"] + extra) == sorted(os.listdir(serial))
    for w in wavs:
        assert open(plain / w, "rb").read() == open(scored / w, "rb").read() == open(serial / w, "rb").read(), w
    for name in extra:
        assert open(scored / name).read() == open(serial / name).read(), name
    # the numbers are Scorer.score's on the pair of files, clip by clip, to the bit
    table = {m: dict(ln.split() for ln in open(scored / f"{m}.scp")) for m in ("SDR", "SISNR", "STOI")}
    uids = [uid for uid, _ in inf_scp if not uid.endswith("_90")]
    assert len(uids) == n16 == 8 and all(list(t) == uids for t in table.values())      # the order of inf.scp
    means = {m: [] for m in table}
    for uid in uids:
        fs, enh = read_wav_f32(str(scored / f"{uid}_enh.wav"))
        _, clean = read_wav_f32(str(clean_dir / f"clean_fileid_{uid.split('fileid_')[-1]}.wav"))
        assert fs == 16000 and enh.shape == clean.shape
        res = scorer.score(torch.from_numpy(clean).cuda(), torch.from_numpy(enh).cuda())
        for m, key in (("SDR", "sdr"), ("SISNR", "sisnr"), ("STOI", "stoi")):
            assert table[m][uid] == repr(float(res[key][0])), (uid, m)
            means[m].append(float(res[key][0]))
    lines = open(scored / "RESULTS.txt").read().splitlines()
    assert lines[:3] == [f"{m}: {np.nanmean(means[m]):.4f}" for m in ("SDR", "SISNR", "STOI")]
    assert len(lines) == 4 and lines[3].startswith("SKIPPED: mix_fileid_90 ") and "PESQ" not in "".join(lines)
