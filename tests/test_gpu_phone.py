"""GPU tests of "telephone-channel rows: exact 8 kHz band + G.711" (csrc/phone.hip through gtcrn_micro_amd.data): the channel
kernel against the numpy statement of the contract (tests/phone_checker.py) BIT FOR BIT -- audio and records -- around the
kernel's chunk, on strides that rule 16-byte accesses out and on strides that allow them, and BatchSource with p_phone=: p_phone
= 0 against the source without it, full draws against the existing checkers followed by the phone checker, ranks, set_step, graph
replay, isolation of a non-finite row.  The contract is integers: nothing below has a tolerance."""
import numpy as np
import pytest

import __graft_entry__ as graft
import active_checker as AC
import batch_checker as BC
import phone_checker as PC

pytestmark = pytest.mark.gpu
CODECS5 = [0, 1, 2, -1, 7]           # one row of each codec, a wide-band row, an entry out of range (counts as -1)
TARGETS = [("narrow", 0), ("wide", 1)]


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def _chunk():
    from gtcrn_micro_amd.data import phone_chunk
    return phone_chunk()


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _nbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


_wants = {}


def _case(L):
    """Five source rows of L samples with their plan and, once computed, the checker's results per target."""
    if L not in _wants:
        n, c = PC.rows_for(L, seed=2)
        n, c = n[[1, 4, 5, 0, 3]], c[[1, 4, 5, 0, 3]]     # loud, full scale, clipped, quiet, the int16 boundaries
        plan = PC.make_plan(CODECS5)
        _wants[L] = (n, c, plan, {tg: PC.phone(n, c, plan, tg) for _, tg in TARGETS})
    return _wants[L]


def _padded(a, stride, lead=0):
    """A host (B, L) array as rows of a NaN-filled (B, stride) device tensor -> (the wide tensor, the view of the rows)."""
    import torch
    B, L = a.shape
    wide = torch.full((B, stride), float("nan"), device="cuda")
    wide[:, lead:lead + L] = torch.from_numpy(a).cuda()
    return wide, wide[:, lead:lead + L]


@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("which", range(6))
def test_kernel_equals_the_checker_bit_for_bit(which, aligned):
    import torch
    from gtcrn_micro_amd.data import phone_channel, phone_plan_to_device
    C = _chunk()
    L = [1, 129, C - 1, C, C + 1, 2 * C + 3][which]
    n, c, plan, wants = _case(L)
    B = len(plan)
    stride = (L + 8) // 4 * 4 if aligned else L + 5      # whole 16 bytes per row, or a stride that rules 16-byte accesses out
    d_plan = phone_plan_to_device(plan, "cuda")
    _, src_n = _padded(n, stride)
    _, src_c = _padded(c, stride)
    clipped = 0
    for name, tg in TARGETS:
        wn, wc, wr = wants[tg]
        wide = [torch.full((B, stride), float("nan"), device="cuda") for _ in range(2)]
        rec = torch.full((B + 1, 4), -9, device="cuda", dtype=torch.int32)
        out_n, out_c, _ = phone_channel(src_n, src_c, d_plan, name, out=(wide[0][:, :L], wide[1][:, :L]), records=rec[:B])
        torch.cuda.synchronize()
        assert rec[:B].cpu().numpy().view(PC.PHONE_RECORD_DTYPE).reshape(B).tobytes() == wr.tobytes(), (name, rec, wr)
        assert bool((rec[B:] == -9).all())
        bad = np.argwhere(_bits(out_n) != _nbits(wn))
        assert bad.size == 0, (name, len(bad), bad[:5])
        bad = np.argwhere(_bits(out_c) != _nbits(wc))
        assert bad.size == 0, (name, len(bad), bad[:5])
        for w in wide:
            assert bool(torch.isnan(w[:, L:]).all()), "the tail of an output row was touched"
        # wide-band rows, and the wide target, are the source bits
        assert np.array_equal(_bits(out_n)[3:], _nbits(n)[3:]) and np.array_equal(_bits(out_c)[3:], _nbits(c)[3:])
        if tg == 1:
            assert np.array_equal(_bits(out_c), _nbits(c))
        clipped += int(wr["saturated_down"].sum()) + int(wr["saturated_up"].sum())
    # the clean pair NULL
    wide = torch.full((B, stride), float("nan"), device="cuda")
    out_n, out_c, rec = phone_channel(src_n, None, d_plan, "narrow", out=wide[:, :L])
    torch.cuda.synchronize()
    assert out_c is None and np.array_equal(_bits(out_n), _nbits(wants[0][0]))
    assert rec.cpu().numpy().view(PC.PHONE_RECORD_DTYPE).reshape(B).tobytes() == wants[0][2].tobytes()
    assert clipped > 0 or L < 64, "no case clipped a sample"


def test_phone_channel_on_a_callers_tensors_equals_the_checker():
    import torch
    from gtcrn_micro_amd.data import phone_channel
    L = 1500
    n, c = PC.rows_for(L, seed=7)
    dn, dc = torch.from_numpy(n).cuda(), torch.from_numpy(c).cuda()
    for name, code in PC.CODECS.items():
        plan = PC.make_plan([code] * len(n))
        for tname, tg in TARGETS:
            wn, wc, wr = PC.phone(n, c, plan, tg)
            on, oc, rec = phone_channel(dn, dc, codec=name, target=tname)
            assert np.array_equal(_bits(on), _nbits(wn)) and np.array_equal(_bits(oc), _nbits(wc))
            assert rec.cpu().numpy().view(PC.PHONE_RECORD_DTYPE).reshape(len(n)).tobytes() == wr.tobytes()
    assert np.array_equal(_bits(dn), _nbits(n)) and np.array_equal(_bits(dc), _nbits(c))      # the inputs are read only
    from gtcrn_micro_amd import GtcrnError
    with pytest.raises(GtcrnError):
        phone_channel(dn, out=dn)                        # in place: refused


def test_a_nan_or_inf_row_changes_no_bit_of_another_row():
    import torch
    from gtcrn_micro_amd.data import phone_channel, phone_plan_to_device
    L = 2 * _chunk() + 3
    n, c = PC.rows_for(L, seed=5)
    plan = phone_plan_to_device(PC.make_plan([0, 1, 2, 1, -1, 2]), "cuda")
    dn, dc = torch.from_numpy(n).cuda(), torch.from_numpy(c).cuda()
    gn, gc, gr = phone_channel(dn, dc, plan, "narrow")
    bn, bc = dn.clone(), dc.clone()
    bn[1, 100], bn[1, L - 2], bc[1, 7] = float("nan"), float("inf"), float("-inf")
    hn, hc, hr = phone_channel(bn, bc, plan, "narrow")
    keep = [0, 2, 3, 4, 5]
    assert torch.equal(hn[keep].view(torch.int32), gn[keep].view(torch.int32))
    assert torch.equal(hc[keep].view(torch.int32), gc[keep].view(torch.int32)) and torch.equal(hr[keep], gr[keep])


# ---- BatchSource ---------------------------------------------------------------------------------------------------------------
def _corpora(seed=3):
    rng = np.random.default_rng(seed)
    speech = [(rng.standard_normal(n) * a).clip(-32768, 32767).astype(np.int16)
              for n, a in ((9000, 6000), (5, 3000), (20000, 12000), (6001, 30000), (7000, 900))]
    noise = [rng.integers(-3000, 3000, n).astype(np.int16) for n in (100, 7000, 3)]
    return speech, noise


def _source(speech, noise, B, L, **kw):
    from gtcrn_micro_amd.data import BatchSource, Corpus
    sp, nz = Corpus.from_arrays(speech), Corpus.from_arrays(noise)
    return BatchSource(sp, noise=nz, B=B, L=L, **kw), sp, nz


def test_p_phone_zero_is_the_source_without_the_argument():
    import torch
    speech, noise = _corpora()
    B, L = 6, 1027
    a, _, _ = _source(speech, noise, B, L, seed=4)
    b, _, _ = _source(speech, noise, B, L, seed=4, p_phone=0.0, phone_codecs=("ulaw",), phone_target="wide")
    assert b.phone_plan is None and b.phone_records is None and not hasattr(b, "_raw_noisy")
    for _ in range(3):
        (an, ac), (bn, bc) = a.draw(), b.draw()
        assert torch.equal(an.view(torch.int32), bn.view(torch.int32)) and torch.equal(ac.view(torch.int32), bc.view(torch.int32))
        assert torch.equal(a.plan, b.plan) and torch.equal(a.records, b.records)
    assert a.step() == b.step() == 3


@pytest.mark.parametrize("target", TARGETS)
def test_mix_then_phone_equals_the_two_checkers_chained(target):
    import torch
    from gtcrn_micro_amd.data import phone_plan_host
    name, tg = target
    speech, noise = _corpora()
    B, L = 16, 2 * _chunk() + 3
    src, sp, nz = _source(speech, noise, B, L, seed=21, p_phone=0.5, phone_target=name)
    soff, noff = sp.offsets.cpu().numpy(), nz.offsets.cpu().numpy()
    for step in range(2):
        noisy, clean = src.draw()
        torch.cuda.synchronize()
        pp = src.phone_plan_numpy()
        assert pp.tobytes() == PC.phone_plan(0.5, 7, B, 21, step).tobytes() == phone_plan_host(0.5, 7, B, 21, step).tobytes()
        assert 0 < int((pp["codec"] >= 0).sum()) < B
        plan = src.plan_numpy()
        BC.assert_same_plan(plan, BC.plan(soff, noff, B, L, 21, step))
        rn, rc, rr = BC.mix(np.concatenate(speech), soff, np.concatenate(noise), noff, plan, L)
        assert src.records_numpy().tobytes() == rr.tobytes()
        assert np.array_equal(_bits(src._raw_noisy), _nbits(rn)) and np.array_equal(_bits(src._raw_clean), _nbits(rc))
        wn, wc, wr = PC.phone(rn, rc, pp, tg)
        assert src.phone_records_numpy().tobytes() == wr.tobytes()
        assert np.array_equal(_bits(noisy), _nbits(wn)) and np.array_equal(_bits(clean), _nbits(wc))
        assert noisy.data_ptr() == src.noisy.data_ptr() and clean.data_ptr() == src.clean.data_ptr()
    assert src.step() == 2


def test_composition_with_reverberation_equals_the_checkers_on_the_staged_corpus():
    import torch
    from gtcrn_micro_amd.data import RirBank
    speech, noise = _corpora(5)
    rng = np.random.default_rng(12)
    rirs = [np.exp(-np.arange(n) / (n / 5.0)) * rng.standard_normal(n) * ([1.0] + [0.3] * (n - 1)) for n in (40, 300, 1)]
    B, L = 6, 1027
    src, sp, nz = _source(speech, noise, B, L, seed=9, rirs=RirBank.from_arrays(rirs), p_reverb=1.0, p_phone=0.6)
    noisy, clean = src.draw()
    torch.cuda.synchronize()
    pp = src.phone_plan_numpy()
    assert pp.tobytes() == PC.phone_plan(0.6, 7, B, 9, 0).tobytes() and 0 < int((pp["codec"] >= 0).sum()) < B
    assert (src.reverb_plan_numpy()["rir"] >= 0).all()
    splan = src.staged_plan.cpu().numpy().view(BC.PLAN_DTYPE).reshape(B)
    rn, rc, rr = BC.mix(src.staged.cpu().numpy(), src.staged_offsets.cpu().numpy(), np.concatenate(noise), nz.offsets.cpu().numpy(),
                        splan, L)
    assert src.records_numpy().tobytes() == rr.tobytes()
    wn, wc, wr = PC.phone(rn, rc, pp, 0)
    assert src.phone_records_numpy().tobytes() == wr.tobytes()
    assert np.array_equal(_bits(noisy), _nbits(wn)) and np.array_equal(_bits(clean), _nbits(wc))


def test_composition_with_active_levels_equals_the_checkers():
    import torch
    from gtcrn_micro_amd.data import active_threshold
    speech, noise = _corpora(6)
    for s in speech:
        s[40:40 + len(s) // 3] = 0
    B, L, W = 6, 1027, 16
    src, sp, nz = _source(speech, noise, B, L, seed=13, active_db=-50.0, active_window=W, p_phone=0.6, phone_codecs=("ulaw", "alaw"))
    noisy, clean = src.draw()
    torch.cuda.synchronize()
    pp = src.phone_plan_numpy()
    assert pp.tobytes() == PC.phone_plan(0.6, 6, B, 13, 0).tobytes() and set(pp["codec"].tolist()) <= {-1, 1, 2}
    assert 0 < int((pp["codec"] >= 0).sum()) < B
    rn, rc, rr = AC.mix_active(np.concatenate(speech), sp.offsets.cpu().numpy(), np.concatenate(noise), nz.offsets.cpu().numpy(),
                               src.plan_numpy(), L, W, active_threshold(-50.0))
    assert src.records_numpy().tobytes() == rr.tobytes()
    wn, wc, wr = PC.phone(rn, rc, pp, 0)
    assert src.phone_records_numpy().tobytes() == wr.tobytes()
    assert np.array_equal(_bits(noisy), _nbits(wn)) and np.array_equal(_bits(clean), _nbits(wc))


def test_pairs_form_with_a_callers_phone_plan():
    import torch
    from gtcrn_micro_amd.data import BatchSource, Corpus, phone_plan_to_device
    speech, _ = _corpora(8)
    cleanc = [(s // 2).astype(np.int16) for s in speech]
    sp, cl = Corpus.from_arrays(speech), Corpus.from_arrays(cleanc)
    B, L = 5, 777
    src = BatchSource(sp, paired_clean=cl, B=B, L=L, seed=2, p_phone=1.0)
    mine = PC.make_plan(CODECS5)
    noisy, clean = src.draw(phone_plan=phone_plan_to_device(mine, "cuda"))
    torch.cuda.synchronize()
    rn, rc = BC.pairs(np.concatenate(speech), np.concatenate(cleanc), sp.offsets.cpu().numpy(), src.plan_numpy(), L)
    wn, wc, wr = PC.phone(rn, rc, mine, 0)
    assert src.phone_records_numpy().tobytes() == wr.tobytes()
    assert np.array_equal(_bits(noisy), _nbits(wn)) and np.array_equal(_bits(clean), _nbits(wc))
    assert src.step() == 1


def test_ranks_cut_one_global_batch_and_set_step_reproduces_a_step():
    import torch
    speech, noise = _corpora()
    L = _chunk() + 1
    whole, _, _ = _source(speech, noise, 16, L, seed=33, p_phone=0.5)
    parts = [_source(speech, noise, 8, L, seed=33, p_phone=0.5, item0=i0)[0] for i0 in (0, 8)]
    kept = []
    for step in range(3):
        n, c = whole.draw()
        kept.append((n.clone(), c.clone(), whole.phone_plan.clone(), whole.phone_records.clone()))
        for k, part in enumerate(parts):
            pn, pc = part.draw()
            rows = slice(8 * k, 8 * k + 8)
            assert torch.equal(pn.view(torch.int32), n[rows].view(torch.int32)) and torch.equal(pc.view(torch.int32), c[rows].view(torch.int32))
            assert torch.equal(part.phone_plan, whole.phone_plan[rows]) and torch.equal(part.phone_records, whole.phone_records[rows])
    assert not torch.equal(kept[0][0], kept[1][0]) and not torch.equal(kept[0][2], kept[2][2])
    whole.set_step(1)
    n, c = whole.draw()
    for got, ref in zip((n, c, whole.phone_plan, whole.phone_records), kept[1]):
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    assert whole.step() == 2


def test_a_captured_draw_replays_consecutive_batches():
    import torch
    speech, noise = _corpora()
    B, L = 6, _chunk() + 1
    eager, _, _ = _source(speech, noise, B, L, seed=5, p_phone=0.5)
    want = []
    for _ in range(2):
        n, c = eager.draw()
        want.append((n.clone(), c.clone(), eager.plan.clone(), eager.records.clone(), eager.phone_plan.clone(), eager.phone_records.clone()))
    src, _, _ = _source(speech, noise, B, L, seed=5, p_phone=0.5)
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
    for k in range(2):
        graph.replay()
        for got, ref in zip((out[0], out[1], src.plan, src.records, src.phone_plan, src.phone_records), want[k]):
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), k
    assert src.step() == 2 and eager.step() == 2
    assert not torch.equal(want[0][0], want[1][0])
