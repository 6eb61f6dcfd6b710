"""GPU tests of "training batches from a resident corpus" (csrc/batch.hip through gtcrn_micro_amd.data): the mix and pairs
draws against the numpy statement of the contract (tests/batch_checker.py) BIT FOR BIT, the device plan against the checker
and against its host twin, row independence, strides, the workspace bound, 64-bit corpus indexing, graph replay and the
hand-off into train_step.  The contract is exact, so nothing below has a tolerance except the 1 ulp on the plan's two pow
results (libm's documented accuracy)."""
import numpy as np
import pytest

import __graft_entry__ as graft
import batch_checker as BC

pytestmark = pytest.mark.gpu
G = 16000


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def _dev_plan(plan):
    from gtcrn_micro_amd.data import plan_to_device
    return plan_to_device(plan, "cuda")


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _records(src):
    return src.records.cpu().numpy().tobytes()


def _corpora(L):
    """Speech and noise clips that put every edge of the contract within reach of an L-sample window."""
    rng = np.random.default_rng(1000 + L)
    r = lambda n, a=12000: rng.integers(-a, a, n).astype(np.int16)      # noqa: E731
    c = r(5000)
    square = np.where(np.arange(5000) % 50 < 25, 32767, -32767).astype(np.int16)
    speech = [r(3), r(9000), r(5), r(6001), np.zeros(5000, np.int16), square, c]       # clip 1 starts at pcm index 3
    one = np.array([-7001], np.int16)
    noise = [one, r(3), r(100), r(L + 5), np.zeros(5000, np.int16), (-c).astype(np.int16), r(7000, 3000)]
    return speech, noise


def _rows(L):
    """(sclip, sstart, nclip, nstart, snr_amp, lvl_amp) and the flags each row must raise (None: not pinned)."""
    rows, flags = [], []

    def add(row, f=None):
        rows.append(row)
        flags.append(f)
    for k in range(9):                                   # windows starting at pcm indices 3 .. 11: every residue mod 8
        add((1, k, 6, 13 + k, 0.5, 0.05))
    add((2, 0, 6, 0, 0.5, 0.05))                         # a 5-sample clip: shorter than the window (unless L < 5)
    add((2, 4, 6, 1, 0.5, 0.05))                         # windows starting at a clip's last sample
    add((1, 8999, 6, 6999, 0.5, 0.05))
    for nc, ln in ((0, 1), (1, 3), (2, 100), (3, L + 5)):   # several wraps, and a wrap inside a 16-byte group
        add((3, 17, nc, ln - 1, 0.7, 0.05))
    add((4, 10, 6, 5, 0.5, 0.05), 2)                     # all-zero speech: noise only
    add((3, 10, 4, 5, 0.5, 0.05), 1)                     # all-zero noise
    add((4, 10, 4, 5, 0.5, 0.05), 1 | 4)                 # both zero
    if L <= 4900:
        add((6, 100, 5, 100, 1.0, 0.05), 4)              # noise = -speech at snr_amp = 1: exact cancellation
    add((5, 3, 4, 0, 1.0, 1.0), 1 | 8)                   # a full-scale square at lvl_amp = 1: the limiter
    add((5, 3, 6, 9, 0.25, 1.0), 8)
    add((3, 1, 6, 2, 1e-6, 0.05))
    add((3, 1, 6, 2, 1e3, 0.05))
    return rows, flags


@pytest.mark.parametrize("L", [1, 7, 8, 9, 255, 1027, 4099])
def test_mix_equals_the_checker_bit_for_bit(L):
    import torch
    from gtcrn_micro_amd.data import BatchSource, Corpus
    speech, noise = _corpora(L)
    rows, flags = _rows(L)
    plan = BC.make_plan(rows)
    sp, nz = Corpus.from_arrays(speech), Corpus.from_arrays(noise)
    src = BatchSource(sp, noise=nz, B=len(rows), L=L)
    noisy, clean = src.draw(plan=_dev_plan(plan))
    torch.cuda.synchronize()
    soff, noff = sp.offsets.cpu().numpy(), nz.offsets.cpu().numpy()
    wn, wc, wr = BC.mix(np.concatenate(speech), soff, np.concatenate(noise), noff, plan, L)
    got = src.records_numpy()
    for b, f in enumerate(flags):
        if f is not None and not (L < 3 and f == 8):     # (a window of one or two samples of the square may not reach the limit)
            assert int(wr["flags"][b]) == f, (b, rows[b], int(wr["flags"][b]))
    assert np.array_equal(got["flags"], wr["flags"]), (got["flags"], wr["flags"])
    assert _records(src) == wr.tobytes()
    assert np.array_equal(_bits(noisy), wn.view(np.int32))
    assert np.array_equal(_bits(clean), wc.view(np.int32))
    assert np.isfinite(wn).all() and np.isfinite(_bits(noisy).view(np.float32)).all()
    # the limiter: |noisy| <= fl(fl(0.99 / peak) * peak), two roundings above 0.99
    lim = [b for b, f in enumerate(wr["flags"]) if f & 8]
    assert lim or L < 3
    top = np.nextafter(np.nextafter(np.float32(0.99), np.float32(1)), np.float32(1))
    for b in lim:
        assert np.abs(_bits(noisy)[b].view(np.float32)).max() <= top
    assert src.step() == 0                               # an explicit plan leaves the step word alone


def test_mix_at_the_workloads_length_chunked_sums_agree_with_a_single_pass():
    import torch
    from gtcrn_micro_amd.data import BatchSource, Corpus
    L = 64000
    rng = np.random.default_rng(7)
    speech = [rng.integers(-20000, 20000, n).astype(np.int16) for n in (5, 70003, 30001)]
    noise = [rng.integers(-9000, 9000, n).astype(np.int16) for n in (100, 64005, 200001)]
    plan = BC.make_plan([(1, 5998, 2, 199999, 0.3, 0.1), (2, 11, 0, 99, 2.0, 0.03), (1, 0, 1, 64004, 1.0, 0.5)])
    sp, nz = Corpus.from_arrays(speech), Corpus.from_arrays(noise)
    src = BatchSource(sp, noise=nz, B=3, L=L)
    noisy, clean = src.draw(plan=_dev_plan(plan))
    torch.cuda.synchronize()
    wn, wc, wr = BC.mix(np.concatenate(speech), sp.offsets.cpu().numpy(), np.concatenate(noise), nz.offsets.cpu().numpy(), plan, L)
    assert _records(src) == wr.tobytes()
    assert np.array_equal(_bits(noisy), wn.view(np.int32)) and np.array_equal(_bits(clean), wc.view(np.int32))


@pytest.mark.parametrize("granule", [1, G])
def test_pairs_equal_numpy_slicing(granule):
    import torch
    from gtcrn_micro_amd.data import BatchSource, Corpus
    L = 4099
    rng = np.random.default_rng(9)
    lens = [1, 3, L - 1, L, L + 1, L + granule, 40000, 2 * L + 7, 52000]
    noisy_c = [rng.integers(-32768, 32768, n).astype(np.int16) for n in lens]
    clean_c = [rng.integers(-32768, 32768, n).astype(np.int16) for n in lens]
    a, c = Corpus.from_arrays(noisy_c), Corpus.from_arrays(clean_c)
    B = 48
    src = BatchSource(a, paired_clean=c, B=B, L=L, seed=77, granule=granule)
    off = a.offsets.cpu().numpy()
    for step in range(2):
        noisy, clean = src.draw()
        torch.cuda.synchronize()
        plan = src.plan_numpy()
        BC.assert_same_plan(plan, BC.plan(off, None, B, L, 77, step, granule=granule))
        wn, wc = BC.pairs(np.concatenate(noisy_c), np.concatenate(clean_c), off, plan, L)
        assert np.array_equal(_bits(noisy), wn.view(np.int32)) and np.array_equal(_bits(clean), wc.view(np.int32))
        assert set(plan["sclip"].tolist()) >= {0, 1, 2}, "the short clips (zero padding) were not drawn"
        assert np.all(plan["sstart"] % granule == 0)
    # explicit starts: a clip's last sample, a window that ends with its clip, clip ids by the caller
    plan = BC.make_plan([(6, 39999, 0, 0, 1, 1), (6, 40000 - L, 0, 0, 1, 1), (8, 5, 0, 0, 1, 1)] * (B // 3))
    noisy, clean = src.draw(plan=_dev_plan(plan))
    wn, wc = BC.pairs(np.concatenate(noisy_c), np.concatenate(clean_c), off, plan, L)
    assert np.array_equal(_bits(noisy), wn.view(np.int32)) and np.array_equal(_bits(clean), wc.view(np.int32))
    clips = torch.arange(B, device="cuda", dtype=torch.int32) % len(lens)
    src.draw(clips=clips)
    assert np.array_equal(src.plan_numpy()["sclip"], clips.cpu().numpy())


@pytest.mark.parametrize("granule", [1, G])
@pytest.mark.parametrize("given", [False, True])
def test_device_plan_equals_the_checker_and_the_host_twin(granule, given):
    import torch
    from gtcrn_micro_amd.data import BatchSource, Corpus, plan_host
    L = 4000
    rng = np.random.default_rng(5)
    slens = [1, L - 1, L, L + 1, L + G, L + 3 * G + 5, 7, 160000] + list(rng.integers(1, 60000, 40))
    nlens = [1, 3, 100, L + 5] + list(rng.integers(1, 20000, 12))
    sp = Corpus.from_arrays([np.zeros(n, np.int16) for n in slens])
    nz = Corpus.from_arrays([np.ones(n, np.int16) for n in nlens])
    soff, noff = sp.offsets.cpu().numpy(), nz.offsets.cpu().numpy()
    B, item0, seed = 300, 1000, 0xfedcba9876543210                      # more than one workgroup of the plan kernel
    clips = (np.arange(B) % 8).astype(np.int32) if given else None
    src = BatchSource(sp, noise=nz, B=B, L=L, seed=seed, granule=granule, item0=item0)
    for step in (0, 1, (1 << 40) + 3):
        src.set_step(step)
        src.draw_plan(clips=None if clips is None else torch.from_numpy(clips).cuda())
        got = src.plan_numpy()
        assert src.step() == step + 1
        BC.assert_same_plan(got, BC.plan(soff, noff, B, L, seed, step, item0=item0, granule=granule, clips=clips))
        BC.assert_same_plan(got, plan_host(soff, noff, B, L, seed, step, item0=item0, granule=granule, clips=clips))
    # item0 enters only through the counter
    one = BatchSource(sp, noise=nz, B=1, L=L, seed=seed, granule=granule, item0=item0 + 3)
    one.set_step(1)
    src.set_step(1)
    src.draw_plan()
    one.draw_plan()
    assert one.plan_numpy().tobytes() == src.plan_numpy()[3:4].tobytes()


def test_rows_are_independent_strides_hold_and_the_workspace_is_bounded():
    import torch
    from gtcrn_micro_amd.data import BatchSource, Corpus, workspace_bytes
    L = 4099
    speech, noise = _corpora(L)
    sp, nz = Corpus.from_arrays(speech), Corpus.from_arrays(noise)
    plan = BC.make_plan([(1, 3, 6, 13, 0.5, 0.05), (2, 0, 2, 99, 0.7, 0.1), (3, 17, 3, L + 4, 2.0, 0.02), (5, 3, 6, 9, 0.25, 1.0),
                         (4, 10, 6, 5, 0.5, 0.05)])
    B = len(plan)
    src = BatchSource(sp, noise=nz, B=B, L=L)
    nbytes = workspace_bytes(B, L)
    assert src._ws.numel() == nbytes
    guard = torch.full((nbytes + 4096,), 0xA5, device="cuda", dtype=torch.uint8)
    src._ws = guard[:nbytes]                            # the same workspace with a guard pattern behind it
    noisy, clean = (t.clone() for t in src.draw(plan=_dev_plan(plan)))
    rec = src.records.clone()
    assert bool((guard[nbytes:] == 0xA5).all()), "the mix wrote past gtcrn_batch_workspace_bytes"
    for b in range(B):
        one = BatchSource(sp, noise=nz, B=1, L=L)
        n1, c1 = one.draw(plan=_dev_plan(plan[b:b + 1]))
        assert torch.equal(n1[0].view(torch.int32), noisy[b].view(torch.int32)), b
        assert torch.equal(c1[0].view(torch.int32), clean[b].view(torch.int32)), b
        assert torch.equal(one.records[0], rec[b]), b
    # rows of wider NaN-filled tensors: a stride that rules 16-byte stores out, one that allows them, rows that start 16 and 12
    # bytes into it
    for stride, lead in ((L + 6, 0), (L + 13, 0), (L + 13, 4), (L + 13, 3)):
        wide = [torch.full((B, stride), float("nan"), device="cuda") for _ in range(2)]
        out = tuple(w[:, lead:lead + L] for w in wide)
        src.draw(plan=_dev_plan(plan), out=out)
        for w, want in zip(wide, (noisy, clean)):
            assert torch.equal(w[:, lead:lead + L].view(torch.int32), want.view(torch.int32)), (stride, lead)
            assert bool(torch.isnan(w[:, :lead]).all()) and bool(torch.isnan(w[:, lead + L:]).all()), (stride, lead)
    # the pairs form under the same strides
    a = Corpus.from_arrays(speech)
    prs = BatchSource(a, paired_clean=Corpus.from_arrays([(-x).clip(-32768, 32767).astype(np.int16) for x in speech]), B=B, L=L)
    pn, pc = (t.clone() for t in prs.draw(plan=_dev_plan(plan)))
    for stride, lead in ((L + 6, 0), (L + 13, 4)):
        wide = [torch.full((B, stride), float("nan"), device="cuda") for _ in range(2)]
        prs.draw(plan=_dev_plan(plan), out=tuple(w[:, lead:lead + L] for w in wide))
        for w, want in zip(wide, (pn, pc)):
            assert torch.equal(w[:, lead:lead + L].view(torch.int32), want.view(torch.int32))
            assert bool(torch.isnan(w[:, :lead]).all()) and bool(torch.isnan(w[:, lead + L:]).all())
    from gtcrn_micro_amd import GtcrnError
    with pytest.raises(GtcrnError):
        src.draw(plan=_dev_plan(plan), out=(noisy[:, :L - 1], clean))


def test_corpus_indexing_is_64_bit():
    """Two clips behind the 2^31-th sample of a 4.3 GB buffer (uninitialised, never read elsewhere) against the same
    clips at offset 0: a 32-bit index would read the buffer's start."""
    import torch
    from gtcrn_micro_amd.data import BatchSource, Corpus
    L = 1027
    rng = np.random.default_rng(3)
    clips = [rng.integers(-15000, 15000, n).astype(np.int16) for n in (1200, 700)]
    small = Corpus.from_arrays(clips)
    base = (1 << 31) + 1
    pcm = torch.empty((1 << 31) + 2 * L, device="cuda", dtype=torch.int16)
    pcm[base:base + 1900] = torch.from_numpy(np.concatenate(clips)).cuda()
    far = Corpus.from_tensors(pcm, torch.tensor([base, base + 1200, base + 1900], device="cuda", dtype=torch.int64))
    plan = _dev_plan(BC.make_plan([(0, 0, 1, 699, 0.5, 0.05), (0, 173, 1, 0, 2.0, 0.1), (1, 5, 0, 1199, 0.5, 0.05), (0, 1199, 0, 7, 1, 1)]))
    for kw_far, kw_small in ((dict(noise=far), dict(noise=small)), (dict(paired_clean=far), dict(paired_clean=small))):
        a = BatchSource(far, B=4, L=L, **kw_far)
        b = BatchSource(small, B=4, L=L, **kw_small)
        (an, ac), (bn, bc) = a.draw(plan=plan), b.draw(plan=plan)
        assert torch.equal(an.view(torch.int32), bn.view(torch.int32)) and torch.equal(ac.view(torch.int32), bc.view(torch.int32))
        assert torch.equal(a.records, b.records)
        assert float(bn.abs().max()) > 0
    del pcm, far, a
    torch.cuda.empty_cache()


def test_a_captured_draw_replays_consecutive_batches():
    import torch
    from gtcrn_micro_amd.data import BatchSource, Corpus
    L, B = 4099, 6
    rng = np.random.default_rng(21)
    sp = Corpus.from_arrays([rng.integers(-9000, 9000, n).astype(np.int16) for n in (9000, 5, 20000, 4099, 6001)])
    nz = Corpus.from_arrays([rng.integers(-3000, 3000, n).astype(np.int16) for n in (100, 7000, 3)])
    eager = BatchSource(sp, noise=nz, B=B, L=L, seed=5)
    want = []
    for _ in range(3):
        n, c = eager.draw()
        want.append((n.clone(), c.clone(), eager.plan.clone(), eager.records.clone()))
    src = BatchSource(sp, noise=nz, B=B, L=L, seed=5)
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
    src.set_step(1)
    n, c = src.draw()
    assert torch.equal(n.view(torch.int32), want[1][0].view(torch.int32)) and torch.equal(c.view(torch.int32), want[1][1].view(torch.int32))
    assert src.step() == 2
    assert not torch.equal(want[0][0], want[1][0]) and not torch.equal(want[1][0], want[2][0])


def test_draw_feeds_train_step_like_the_checkers_arrays():
    import torch
    from gtcrn_micro_amd.data import BatchSource, Corpus
    from gtcrn_micro_amd.train import make_training, resident_epoch, train_step
    L, B = 4096, 2                                       # the smallest shape of the train tests (synthetic_mix(2, 4096))
    rng = np.random.default_rng(4)
    speech = [(3000 * np.sin(np.arange(n) * 0.05 * (k + 1)) + rng.integers(-200, 200, n)).astype(np.int16) for k, n in enumerate((9000, 5000, 4096))]
    noise = [rng.integers(-3000, 3000, n).astype(np.int16) for n in (100, 7000)]
    sp, nz = Corpus.from_arrays(speech), Corpus.from_arrays(noise)
    src = BatchSource(sp, noise=nz, B=B, L=L, seed=8)
    cfg = {"warmup_steps": 5, "decay_until_step": 100}

    def fresh():
        torch.manual_seed(43)
        m, o, s, lf = make_training(cfg, device="cuda")
        m.train()
        return m, o, s, lf
    ma, oa, sa, la = fresh()
    noisy, clean = src.draw()
    l1, g1 = train_step(ma, oa, sa, la, noisy, clean)
    plan = src.plan_numpy()
    wn, wc, _ = BC.mix(np.concatenate(speech), sp.offsets.cpu().numpy(), np.concatenate(noise), nz.offsets.cpu().numpy(), plan, L)
    mb, ob, sb, lb = fresh()
    l2, g2 = train_step(mb, ob, sb, lb, torch.from_numpy(wn).cuda(), torch.from_numpy(wc).cuda())
    assert np.isfinite(float(l1)) and float(g1) > 0
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32)) and torch.equal(g1.view(torch.int32), g2.view(torch.int32))
    # resident_epoch is that loop: its first step from step word 0 is the step above
    mc, oc, sc, lc = fresh()
    src.set_step(0)
    losses, norms = resident_epoch(src, 2, mc, oc, sc, lc)
    assert losses.shape == (2,) and norms.shape == (2,) and src.step() == 2
    assert torch.equal(losses[0].view(torch.int32), l1.view(torch.int32)) and torch.equal(norms[0].view(torch.int32), g1.view(torch.int32))


def test_corpus_round_trips_through_wav_files_and_the_npy_pair(tmp_path):
    import torch
    from gtcrn_micro_amd.data import Corpus
    from gtcrn_micro_amd.infer import write_wav_pcm16
    rng = np.random.default_rng(2)
    clips = [rng.integers(-32768, 32768, n).astype(np.int16) for n in (1, 1601, 16000)]
    paths = []
    for k, c in enumerate(clips):
        paths.append(str(tmp_path / f"clip{k}.wav"))
        write_wav_pcm16(paths[-1], c.astype(np.float32) / 32768.0)          # exact: int16 / 32768 and back
    a, b = Corpus.from_arrays(clips), Corpus.from_wavs(paths)
    assert a.n == b.n == 3 and torch.equal(a.pcm, b.pcm) and torch.equal(a.offsets, b.offsets)
    assert a.offsets.cpu().tolist() == [0, 1, 1602, 17602]
    b.save(str(tmp_path / "corpus"))
    c = Corpus.load(str(tmp_path / "corpus"))
    assert torch.equal(c.pcm, a.pcm) and torch.equal(c.offsets, a.offsets) and c.pcm.is_cuda
