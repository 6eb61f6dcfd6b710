"""GPU tests of "active levels" (the three active kernels of csrc/batch.hip through gtcrn_micro_amd.data): the draw against the
numpy statement of the contract (tests/active_checker.py) BIT FOR BIT -- records, noisy and clean --, its equality with the plain
draw where every window is active, chunked rows, the composition with reverberation and targets, row independence, strides, the
workspace bound, graph replay and the `passes` subsets.  The contract is exact: nothing below has a tolerance."""
import numpy as np
import pytest

import __graft_entry__ as graft
import active_checker as AC
import batch_checker as BC

pytestmark = pytest.mark.gpu
THR = 10000                                              # int16^2 mean square: -50.3 dB re full scale; a window of 100s ties
THR_DB = 10.0 * np.log10(10000.5 / 2.0 ** 30)            # active_threshold(THR_DB) == THR


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def _dev_plan(plan):
    from gtcrn_micro_amd.data import plan_to_device
    return plan_to_device(plan, "cuda")


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _corpora(L, W):
    """test_gpu_batch's clips (every edge of the plain contract within reach of an L-sample window: clips 0 .. 6 of each side)
    and, behind them, the clips that put the edges of the activity rule within reach."""
    rng = np.random.default_rng(1000 + L)
    r = lambda n, a=12000: rng.integers(-a, a, n).astype(np.int16)      # noqa: E731
    c = r(5000)
    square = np.where(np.arange(5000) % 50 < 25, 32767, -32767).astype(np.int16)
    speech = [r(3), r(9000), r(5), r(6001), np.zeros(5000, np.int16), square, c]       # clip 1 starts at pcm index 3
    one = np.array([-7001], np.int16)
    noise = [one, r(3), r(100), r(L + 5), np.zeros(5000, np.int16), (-c).astype(np.int16), r(7000, 3000)]

    def gappy(n, a):                                     # a silent stretch of 2.5 windows: a whole window of any row inside it
        x = r(n, a)
        x[W:W + 5 * W // 2] = 0
        return x

    def tie(n, v):                                       # the first window exactly at the threshold, the rest above it
        x = np.full(n, v, np.int16)
        x[:W] = 100
        return x
    loud = r(L % W + 40)
    loud = np.where(loud >= 0, loud // 2 + 3000, loud // 2 - 3000).astype(np.int16)
    last = np.concatenate([np.zeros(L // W * W, np.int16), loud])                       # only the short last window is loud
    speech += [gappy(L + 3 * W + 50, 12000), tie(L + W, 101), r(L + 10, 50), last]      # clips 7 .. 10
    noise += [gappy(L + 57, 3000), tie(L + W, -101), r(300, 50)]                        # clips 7 .. 9
    return speech, noise


def _rows(L):
    """(sclip, sstart, nclip, nstart, snr_amp, lvl_amp), the flags 1 | 2 | 4 | 8 each row must raise and the flags 16 | 32
    (None: not pinned)."""
    rows, flags, inactive = [], [], []

    def add(row, f=None, a=None):
        rows.append(row)
        flags.append(f)
        inactive.append(a)
    for k in range(9):                                   # windows starting at pcm indices 3 .. 11: every residue mod 8
        add((1, k, 6, 13 + k, 0.5, 0.05))
    add((2, 0, 6, 0, 0.5, 0.05))                         # a 5-sample clip: shorter than the window (unless L < 5)
    add((2, 4, 6, 1, 0.5, 0.05))                         # windows starting at a clip's last sample
    add((1, 8999, 6, 6999, 0.5, 0.05))
    for nc, ln in ((0, 1), (1, 3), (2, 100), (3, L + 5)):   # several wraps, and a wrap inside a 16-byte group
        add((3, 17, nc, ln - 1, 0.7, 0.05))
    add((4, 10, 6, 5, 0.5, 0.05), 2, 16)                 # all-zero speech: noise only
    add((3, 10, 4, 5, 0.5, 0.05), 1, 32)                 # all-zero noise
    add((4, 10, 4, 5, 0.5, 0.05), 1 | 4, 48)             # both zero
    if L <= 4900:
        add((6, 100, 5, 100, 1.0, 0.05), 4)              # noise = -speech at snr_amp = 1: exact cancellation
    add((5, 3, 4, 0, 1.0, 1.0), 1 | 8, 32)               # a full-scale square at lvl_amp = 1: the limiter
    add((5, 3, 6, 9, 0.25, 1.0), 8)
    add((3, 1, 6, 2, 1e-6, 0.05))
    add((3, 1, 6, 2, 1e3, 0.05))
    # the activity rule
    add((7, 0, 6, 3, 0.5, 0.05))                         # speech with a silent stretch longer than a window
    add((7, 5, 7, 11, 0.5, 0.05))                        # ... against noise with one, both off the window grid
    add((1, 2, 7, 0, 0.7, 0.05))                         # noise with a silent stretch
    add((8, 0, 7, 0, 0.5, 0.05))                         # partly active on both sides, over different numbers of samples
    add((8, 0, 6, 1, 0.5, 0.05))                         # a speech window exactly at the threshold
    add((1, 0, 8, 0, 0.5, 0.05))                         # a noise window exactly at the threshold
    add((9, 3, 6, 5, 0.5, 0.05), None, 16)               # no speech window is active
    add((1, 1, 9, 7, 0.5, 0.05), None, 32)               # no noise window is active
    add((9, 0, 9, 0, 0.5, 0.05), None, 48)               # neither
    add((10, 0, 6, 0, 0.5, 0.05))                        # the short last window is the only active one
    return rows, flags, inactive


def _source(speech, noise, B, L, W, **kw):
    from gtcrn_micro_amd.data import BatchSource, Corpus
    sp, nz = Corpus.from_arrays(speech), Corpus.from_arrays(noise)
    src = BatchSource(sp, noise=nz, B=B, L=L, active_db=THR_DB, active_window=W, **kw)
    assert src.active_threshold == THR and tuple(src.records.shape) == (B, 16)
    return src, sp, nz


@pytest.mark.parametrize("L,W", [(1, 16), (7, 16), (8, 16), (9, 16), (17, 16), (255, 16), (1027, 16), (4099, 16), (4099, 8), (4099, 1600)])
def test_active_mix_equals_the_checker_bit_for_bit(L, W):
    import torch
    speech, noise = _corpora(L, W)
    rows, flags, inactive = _rows(L)
    plan = BC.make_plan(rows)
    src, sp, nz = _source(speech, noise, len(rows), L, W)
    noisy, clean = src.draw(plan=_dev_plan(plan))
    torch.cuda.synchronize()
    soff, noff = sp.offsets.cpu().numpy(), nz.offsets.cpu().numpy()
    wn, wc, wr = AC.mix_active(np.concatenate(speech), soff, np.concatenate(noise), noff, plan, L, W, THR)
    # what the rows are for, on the checker's own records: the test cannot pass vacuously
    for b, (f, a) in enumerate(zip(flags, inactive)):
        if f is not None and not (L < 3 and f & 8):      # (a window of one or two samples of the square may not reach the limit)
            assert int(wr["flags"][b]) & 15 == f, (b, rows[b], int(wr["flags"][b]))
        if a is not None and L >= 17:                    # (one small sample can lie below the threshold)
            assert int(wr["flags"][b]) & 48 == a, (b, rows[b], int(wr["flags"][b]))
    some_s = (wr["Ns"] > 0) & (wr["Ns"] < L) & (wr["flags"] & 16 == 0)
    some_n = (wr["Nn"] > 0) & (wr["Nn"] < L) & (wr["flags"] & 32 == 0)
    if L >= 17:
        assert some_s.sum() >= 3 and some_n.sum() >= 2, (wr["Ns"], wr["Nn"])
        assert (some_s & some_n & (wr["Ns"] != wr["Nn"])).any()              # the Nn / Ns factor is in play
        last = len(rows) - 1
        assert wr["Ns"][last] == L % W and wr["As"][last] == wr["Ss"][last]  # the short last window alone
        tie_s, tie_n = len(rows) - 6, len(rows) - 5
        assert wr["Ns"][tie_s] == L - W and wr["Nn"][tie_n] == L - W          # the window at the threshold is inactive
    assert ((wr["Ns"] == L) & (wr["Nn"] == L) & (wr["flags"] & 48 == 0)).any()
    got = src.records_numpy()
    assert got.dtype == AC.ACTIVE_RECORD_DTYPE
    for f in ("flags", "Ns", "Nn", "As", "An", "Ss", "Sn", "Ssn"):
        assert np.array_equal(got[f], wr[f]), (f, got[f], wr[f])
    assert got.tobytes() == wr.tobytes()
    assert np.array_equal(_bits(noisy), wn.view(np.int32))
    assert np.array_equal(_bits(clean), wc.view(np.int32))
    assert np.isfinite(wn).all() and np.isfinite(wc).all()
    assert src.step() == 0                               # an explicit plan leaves the step word alone


@pytest.mark.parametrize("L,W", [(1027, 16), (4099, 1600)])
def test_with_every_window_active_the_draw_is_the_plain_draw(L, W):
    import torch
    from gtcrn_micro_amd.data import BatchSource, Corpus
    rng = np.random.default_rng(L)
    nz_free = lambda n, a: (rng.integers(1, a, n) * rng.choice([-1, 1], n)).astype(np.int16)      # noqa: E731
    sp = Corpus.from_arrays([nz_free(n, 12000) for n in (L, L + 1, 2 * L + 3, 9000)])
    nz = Corpus.from_arrays([nz_free(n, 3000) for n in (1, 3, 100, L + 5, 7000)])
    B = 8
    plain = BatchSource(sp, noise=nz, B=B, L=L, seed=3)
    act = BatchSource(sp, noise=nz, B=B, L=L, seed=3, active_db=float("-inf"), active_window=W)
    assert act.active_threshold == 0
    for _ in range(2):
        pn, pc = plain.draw()
        an, ac = act.draw()
        torch.cuda.synchronize()
        assert torch.equal(plain.plan, act.plan)
        assert torch.equal(an.view(torch.int32), pn.view(torch.int32)) and torch.equal(ac.view(torch.int32), pc.view(torch.int32))
        p, a = plain.records_numpy(), act.records_numpy()
        for f in ("Ss", "Sn", "Ssn", "flags"):
            assert np.array_equal(p[f], a[f]), f
        for f in ("gn", "Gf", "peak"):
            assert np.array_equal(p[f].view(np.int32), a[f].view(np.int32)), f
        assert np.all(a["Ns"] == L) and np.all(a["Nn"] == L)
        assert np.array_equal(a["As"], a["Ss"]) and np.array_equal(a["An"], a["Sn"])


def _long_rows(L, W, B):
    rng = np.random.default_rng(7)
    speech = [rng.integers(-20000, 20000, n).astype(np.int16) for n in (5, L + 6003, L // 2 + 1)]
    for s in speech[1:]:                                 # pauses: digital silence and a level below the threshold
        s[3 * W + 5:9 * W] = 0
        s[L // 3:L // 3 + 4 * W + 3] = rng.integers(-60, 60, 4 * W + 3)
    noise = [rng.integers(-9000, 9000, n).astype(np.int16) for n in (100, L + 5, 3 * L + 1)]
    noise[2][10 * W:16 * W] = 0
    rows = [(1, 5998, 2, 3 * L, 0.3, 0.1), (2, 11, 0, 99, 2.0, 0.03), (1, 0, 1, L + 4, 1.0, 0.5)][:B]
    return speech, noise, BC.make_plan(rows)


@pytest.mark.parametrize("L,W,B,chunks", [(64000, 1600, 3, 14), (64000, 8, 3, 16), (256 * 4800 - 7, 1600, 1, 256)])
def test_chunked_partials_agree_with_a_single_pass(L, W, B, chunks):
    """Rows of 14 and 16 chunks at the workload's length, and one row of MAX_CHUNKS chunks (every thread of the passes that
    add an item's partials up holds one), against the checker's single pass."""
    import torch
    from gtcrn_micro_amd.data import active_workspace_bytes
    speech, noise, plan = _long_rows(L, W, B)
    assert active_workspace_bytes(B, L, W) == (B * chunks * 60 + 15) // 16 * 16
    src, sp, nz = _source(speech, noise, B, L, W)
    noisy, clean = src.draw(plan=_dev_plan(plan))
    torch.cuda.synchronize()
    wn, wc, wr = AC.mix_active(np.concatenate(speech), sp.offsets.cpu().numpy(), np.concatenate(noise), nz.offsets.cpu().numpy(), plan,
                               L, W, THR)
    assert np.all((wr["Ns"] > 0) & (wr["Ns"] < L)) and np.any((wr["Nn"] > 0) & (wr["Nn"] < L))
    assert src.records_numpy().tobytes() == wr.tobytes()
    assert np.array_equal(_bits(noisy), wn.view(np.int32)) and np.array_equal(_bits(clean), wc.view(np.int32))


@pytest.fixture(scope="module")
def _reverb_setup():
    from gtcrn_micro_amd.data import Corpus, RirBank
    rng = np.random.default_rng(12)
    speech = [rng.integers(-12000, 12000, n).astype(np.int16) for n in (9000, 5, 1500, 2600)]
    for s in (speech[0], speech[3]):
        s[200:700] = 0                                   # pauses for the responses' tails to fall into
    noise = [rng.integers(-3000, 3000, n).astype(np.int16) for n in (100, 7000, 50)]
    noise[0][20:60], noise[1][300:900], noise[2][5:45] = 0, 0, 0      # a silent stretch of more than two windows in each
    target = [(s // 2 + rng.integers(-50, 50, len(s))).astype(np.int16) for s in speech]
    rirs = [np.exp(-np.arange(n) / (n / 5.0)) * rng.standard_normal(n) * ([1.0] + [0.3] * (n - 1)) for n in (40, 300, 1)]
    return (speech, noise, target, Corpus.from_arrays(speech), Corpus.from_arrays(noise), Corpus.from_arrays(target),
            RirBank.from_arrays(rirs))


@pytest.mark.parametrize("form", ["rirs", "rirs_target_ms", "target"])
def test_composition_with_reverberation_and_targets_equals_the_checker_on_the_staged_corpora(form, _reverb_setup):
    import torch
    from gtcrn_micro_amd.data import BatchSource
    speech, noise, target, sp, nz, tg, bank = _reverb_setup
    B, L, W = 4, 1027, 16
    kw = {"rirs": dict(rirs=bank, p_reverb=1.0), "rirs_target_ms": dict(rirs=bank, p_reverb=1.0, target_ms=2), "target": dict(target=tg)}[form]
    src = BatchSource(sp, noise=nz, B=B, L=L, seed=9, active_db=THR_DB, active_window=W, **kw)
    noff = nz.offsets.cpu().numpy()
    for _ in range(2):
        noisy, clean = src.draw()
        torch.cuda.synchronize()
        if form == "target":
            spcm, soff, plan, tpcm = np.concatenate(speech), sp.offsets.cpu().numpy(), src.plan_numpy(), np.concatenate(target)
        else:
            assert (src.reverb_plan_numpy()["rir"] >= 0).all()
            spcm, soff = src.staged.cpu().numpy(), src.staged_offsets.cpu().numpy()
            plan = src.staged_plan.cpu().numpy().view(BC.PLAN_DTYPE).reshape(B)
            tpcm = src.staged_target.cpu().numpy() if form == "rirs_target_ms" else None
        wn, wc, wr = AC.mix_active(spcm, soff, np.concatenate(noise), noff, plan, L, W, THR, tpcm=tpcm)
        assert src.records_numpy().tobytes() == wr.tobytes()
        assert np.array_equal(_bits(noisy), wn.view(np.int32)) and np.array_equal(_bits(clean), wc.view(np.int32))
        assert np.any(wr["Ns"] < L) or np.any(wr["Nn"] < L)
        if tpcm is not None:
            plain_clean = AC.mix_active(spcm, soff, np.concatenate(noise), noff, plan, L, W, THR)[1]
            assert not np.array_equal(plain_clean, wc), "the target does not differ from the speech side"
    assert src.step() == 2


def test_rows_are_independent_strides_hold_and_the_workspace_is_bounded():
    import torch
    from gtcrn_micro_amd.data import active_workspace_bytes
    L, W = 4099, 16
    speech, noise = _corpora(L, W)
    plan = BC.make_plan([(1, 3, 6, 13, 0.5, 0.05), (7, 5, 7, 11, 0.7, 0.1), (9, 3, 3, L + 4, 2.0, 0.02), (5, 3, 6, 9, 0.25, 1.0),
                         (4, 10, 6, 5, 0.5, 0.05), (10, 0, 9, 0, 0.5, 0.05)])
    B = len(plan)
    src, sp, nz = _source(speech, noise, B, L, W)
    nbytes = active_workspace_bytes(B, L, W)
    assert src._ws.numel() == nbytes
    guard = torch.full((nbytes + 4096,), 0xA5, device="cuda", dtype=torch.uint8)
    src._ws = guard[:nbytes]                            # the same workspace with a guard pattern behind it
    noisy, clean = (t.clone() for t in src.draw(plan=_dev_plan(plan)))
    rec = src.records.clone()
    assert bool((guard[nbytes:] == 0xA5).all()), "the active mix wrote past gtcrn_batch_active_workspace_bytes"
    # a row alone, and the row beside another clip in the neighbouring row: not a bit of it changes
    for b in range(B):
        one, _, _ = _source(speech, noise, 1, L, W)
        n1, c1 = one.draw(plan=_dev_plan(plan[b:b + 1]))
        assert torch.equal(n1[0].view(torch.int32), noisy[b].view(torch.int32)), b
        assert torch.equal(c1[0].view(torch.int32), clean[b].view(torch.int32)), b
        assert torch.equal(one.records[0], rec[b]), b
    other = plan.copy()
    other["sclip"][1], other["sstart"][1], other["nclip"][1] = 3, 17, 2
    n2, c2 = src.draw(plan=_dev_plan(other))
    keep = [0, 2, 3, 4, 5]
    assert torch.equal(n2[keep].view(torch.int32), noisy[keep].view(torch.int32)) and torch.equal(src.records[keep], rec[keep])
    assert torch.equal(c2[keep].view(torch.int32), clean[keep].view(torch.int32)) and not torch.equal(n2[1], noisy[1])
    # rows of wider NaN-filled tensors: a stride that rules 16-byte stores out, one that allows them, rows that start 16 and 12
    # bytes into it
    for stride, lead in ((L + 6, 0), (L + 13, 0), (L + 13, 4), (L + 13, 3)):
        wide = [torch.full((B, stride), float("nan"), device="cuda") for _ in range(2)]
        out = tuple(w[:, lead:lead + L] for w in wide)
        src.draw(plan=_dev_plan(plan), out=out)
        for w, want in zip(wide, (noisy, clean)):
            assert torch.equal(w[:, lead:lead + L].view(torch.int32), want.view(torch.int32)), (stride, lead)
            assert bool(torch.isnan(w[:, :lead]).all()) and bool(torch.isnan(w[:, lead + L:]).all()), (stride, lead)


def test_a_captured_active_draw_replays_consecutive_batches():
    import torch
    L, B, W = 4099, 6, 16
    rng = np.random.default_rng(21)
    speech = [rng.integers(-9000, 9000, n).astype(np.int16) for n in (9000, 5, 20000, 4099, 6001)]
    for s in speech:
        s[40:40 + len(s) // 3] = 0
    noise = [rng.integers(-3000, 3000, n).astype(np.int16) for n in (100, 7000, 3)]
    eager, _, _ = _source(speech, noise, B, L, W, seed=5)
    want = []
    for _ in range(3):
        n, c = eager.draw()
        want.append((n.clone(), c.clone(), eager.plan.clone(), eager.records.clone()))
    assert any(np.any(w[3].cpu().numpy().view(AC.ACTIVE_RECORD_DTYPE)["Ns"] < L) for w in want)
    src, _, _ = _source(speech, noise, B, L, W, seed=5)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        src.draw()                                      # warm-up outside the capture
        src.set_step(0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = src.draw()
    assert src.step() == 0                              # captured, not run
    for k in range(3):
        graph.replay()
        for got, ref in zip((out[0], out[1], src.plan, src.records), want[k]):
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), k
    assert src.step() == 3 and eager.step() == 3
    assert not torch.equal(want[0][0], want[1][0]) and not torch.equal(want[1][0], want[2][0])


def test_passes_run_separately_give_the_bytes_of_a_whole_draw():
    import torch
    L, W = 4099, 16
    speech, noise = _corpora(L, W)
    rows, _, _ = _rows(L)
    plan = _dev_plan(BC.make_plan(rows))
    whole, _, _ = _source(speech, noise, len(rows), L, W)
    wn, wc = whole.draw(plan=plan)
    parts, _, _ = _source(speech, noise, len(rows), L, W)
    parts.noisy.fill_(float("nan"))
    parts.clean.fill_(float("nan"))
    for p in (1, 2, 4):
        pn, pc = parts.draw(plan=plan, passes=p)
        if p != 4:
            assert bool(torch.isnan(pn).all()) and not bool(parts.records.any()), "a pass before the write wrote rows or records"
    torch.cuda.synchronize()
    assert torch.equal(pn.view(torch.int32), wn.view(torch.int32)) and torch.equal(pc.view(torch.int32), wc.view(torch.int32))
    used = len(rows) * 2 * 60                            # two chunks per row, seven int64 sums and a float peak per chunk
    assert torch.equal(parts.records, whole.records) and torch.equal(parts._ws[:used], whole._ws[:used])
