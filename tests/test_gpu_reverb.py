"""GPU tests of "reverberant speech: exact RIR convolution" (csrc/reverb.hip through gtcrn_micro_amd.data): the int8 MFMA lane
maps, both forms of the convolution against the numpy statement of the contract (tests/reverb_checker.py) BIT FOR BIT --
staged samples, offsets, rewritten plan and records -- around the 16-output tile, the 64-tap chunk and the 2048- and
8192-sample blocks, and BatchSource with rirs=: p_reverb = 0 against the source without a bank, full draws against the two checkers
chained, graph replay, clamped plans.  The contract is exact: nothing below has a tolerance except the 1 ulp on the batch
plan's two pow results that tests/test_gpu_batch.py allows as well."""
import os

import numpy as np
import pytest

from conftest import ROOT

import __graft_entry__ as graft
import batch_checker as BC
import reverb_checker as RC

pytestmark = pytest.mark.gpu
BLOCK, BIG_BLOCK = 2048, 8192      # gtr::BLOCK, gtr::BIG_BLOCK: output samples of one workgroup
FORMS = [1, 3, 4]                  # plain; matrix with the small and with the large block (form 2 is one of these by the shape)
GUARD = 0x5A5A
KS = [1, 15, 16, 17, 63, 64, 65, 1000, 16384]
LS = [1, 15, 16, 17, 255, BLOCK - 1, BLOCK + 1]
LS_BIG = [BIG_BLOCK - 1, BIG_BLOCK + 1]


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def test_selftest_mfma_i8():
    from gtcrn_micro_amd import selftest_mfma_i8
    selftest_mfma_i8(0)


class _Setup:
    """Corpus and bank on the device, with their host copies."""

    def __init__(self, speech, rirs):
        from gtcrn_micro_amd.data import Corpus, RirBank
        self.speech, self.rirs = speech, rirs
        self.sp = Corpus.from_arrays(speech)
        self.bank = RirBank.from_arrays(rirs, trim_direct=False)
        self.spcm, self.soff = np.concatenate(speech), self.sp.offsets.cpu().numpy()
        self.taps, self.roff = np.concatenate(rirs), self.bank.offsets.cpu().numpy()
        assert np.array_equal(self.bank.taps.cpu().numpy(), self.taps)       # int16 taps are taken as they stand

    def want(self, plan, rplan, L, stride):
        return RC.reverb(self.spcm, self.soff, self.taps, self.roff, plan, rplan, L, stride)

    def run(self, plan, rplan, L, stride, form, sp=None):
        """gtcrn_batch_reverb on guarded buffers -> (staged (B, stride), offsets, staged plan, records), all numpy."""
        import torch
        from gtcrn_micro_amd._lib import _check, lib
        from gtcrn_micro_amd.data import plan_to_device, reverb_plan_to_device, reverb_workspace_bytes
        sp = sp or self.sp
        B = len(plan)
        staged = torch.full((B * stride + 64,), GUARD, device="cuda", dtype=torch.int16)
        so = torch.full((B + 3,), -7, device="cuda", dtype=torch.int64)
        splan = torch.full((B + 1, 8), -3, device="cuda", dtype=torch.int32)
        rec = torch.full((B + 1, 4), -9, device="cuda", dtype=torch.int32)
        nws = reverb_workspace_bytes(B, L)
        ws = torch.full((nws + 256,), 0xA5, device="cuda", dtype=torch.uint8)
        p, rp = plan_to_device(plan, "cuda"), reverb_plan_to_device(rplan, "cuda")
        bk = self.bank
        _check(lib().gtcrn_batch_reverb(sp.pcm.data_ptr(), sp.offsets.data_ptr(), sp.n, bk.taps.data_ptr(), bk.offsets.data_ptr(), bk.n,
                                        bk.table.data_ptr() if form != 1 else None, bk.table.numel(), p.data_ptr(), rp.data_ptr(), B, L,
                                        staged.data_ptr(), stride, so.data_ptr(), splan.data_ptr(), rec.data_ptr(), ws.data_ptr(),
                                        form, None))
        torch.cuda.synchronize()
        assert bool((staged[B * stride:] == GUARD).all()), "wrote behind the staged corpus"
        assert bool((so[B + 1:] == -7).all()) and bool((splan[B:] == -3).all()) and bool((rec[B:] == -9).all())
        assert bool((ws[nws:] == 0xA5).all()), "wrote past gtcrn_batch_reverb_workspace_bytes"
        return (staged[:B * stride].cpu().numpy().reshape(B, stride), so[:B + 1].cpu().numpy(),
                splan[:B].cpu().numpy().view(BC.PLAN_DTYPE).reshape(B), rec[:B].cpu().numpy().view(RC.REVERB_RECORD_DTYPE).reshape(B))

    def check(self, plan, rplan, L, stride, form, want=None, sp=None):
        ws, wo, wp, wr = want or self.want(plan, rplan, L, stride)
        gs, go, gp, gr = self.run(plan, rplan, L, stride, form, sp)
        assert gr.tobytes() == wr.tobytes(), (gr, wr)
        bad = np.argwhere(gs[:, :L] != ws[:, :L])
        assert bad.size == 0, (len(bad), bad[:5], gs[:, :L][tuple(bad[0])], ws[:, :L][tuple(bad[0])])
        assert np.all(gs[:, L:] == GUARD), "the tail of a staged row was touched"
        assert np.array_equal(go, wo) and gp.tobytes() == wp.tobytes()
        return wr


def _plan(rows):
    """rows of (sclip, sstart): the other fields of a batch item only pass through the convolution."""
    return BC.make_plan([(c, s, 3 + b, 11 * b, 0.25 + b, 0.05 * (b + 1)) for b, (c, s) in enumerate(rows)])


_cases = {}


def _case(K):
    """The set-up of one K and, once computed, its expected results (shared by both forms)."""
    if K not in _cases:
        rng = np.random.default_rng(100 + K)
        n = 2 * K + 4200
        long_ = rng.integers(-32768, 32768, n).astype(np.int16)
        long_[K:K + 4] = [32767, -32768, 32767, -32768]
        speech = [rng.integers(-32768, 32768, 9).astype(np.int16), long_, rng.integers(-32768, 32768, max(1, K // 2)).astype(np.int16)]
        loud = rng.integers(-RC.TAP_MAX, RC.TAP_MAX + 1, K).astype(np.int16)
        loud[0], loud[-1] = RC.TAP_MAX, -RC.TAP_MAX if K > 1 else RC.TAP_MAX
        quiet = (loud // 64).astype(np.int16)                                # the same length: sums that seldom clamp
        _cases[K] = (_Setup(speech, [loud, quiet, np.array([20000, -9000, 4000], np.int16)]), {})
    return _cases[K]


def _batches(K, L):
    n = 2 * K + 4200
    odd = L + 5 if (L + 5) % 4 else L + 6
    return [
        # one clip, starts with the whole history inside the clip (K - 1, K, K + 1) and with zeros before it (0, 1); rows sharing a response
        (_plan([(1, 0), (1, 1), (1, K - 1), (1, K), (1, K + 1)]), RC.make_reverb_plan([0, 0, 1, 0, 1]), (L + 3) // 4 * 4),
        # a clip shorter than the window (its tail rings into the padding), dry rows between wet ones, a clip shorter than the
        # response, a window that leaves its clip, under a stride above L that rules 8-byte stores out
        (_plan([(0, 0), (1, 7), (2, 0), (1, n - 3), (1, n - 2)]), RC.make_reverb_plan([0, -1, 1, -1, 2]), odd),
        (_plan([(1, K + 2)]), RC.make_reverb_plan([0]), L),
    ]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("K", KS)
def test_both_forms_equal_the_checker_bit_for_bit(K, form):
    st, wants = _case(K)
    clamped = 0
    for L in LS + (LS_BIG if form == 4 else []):
        for k, (plan, rplan, stride) in enumerate(_batches(K, L)):
            if L > BIG_BLOCK - 2 and K > 1000 and k != 2:
                continue                                 # (the large block's edge at 16384 taps: the one-row batch)
            if (L, k) not in wants:
                wants[(L, k)] = st.want(plan, rplan, L, stride)
            rec = st.check(plan, rplan, L, stride, form, wants[(L, k)])
            clamped += int(rec["saturated"].sum())
            assert np.array_equal(rec["ntaps"], np.where(rplan["rir"] < 0, 0, np.where(rplan["rir"] == 2, 3, K)))
    assert clamped > 0 or K == 1, "no case clamped a sample"


@pytest.mark.parametrize("form", FORMS)
def test_extreme_speech_against_extreme_taps_at_16384_taps(form):
    """The largest digit sums: speech all 32767 / all -32768 against taps all at the bank's maximum / minimum."""
    K, L = RC.MAX_TAPS, BLOCK + 1
    if "extreme" not in _cases:
        speech = [np.full(K + L, 32767, np.int16), np.full(K + L, -32768, np.int16)]
        st = _Setup(speech, [np.full(K, RC.TAP_MAX, np.int16), np.full(K, -RC.TAP_MAX, np.int16)])
        plan, rplan = _plan([(0, K), (0, K), (1, K), (1, K), (1, 0)]), RC.make_reverb_plan([0, 1, 0, 1, 0])
        _cases["extreme"] = (st, plan, rplan, st.want(plan, rplan, L, L + 3))
    st, plan, rplan, want = _cases["extreme"]
    rec = st.check(plan, rplan, L, L + 3, form, want)
    assert rec["saturated"].tolist() == [L, L, L, L, L - 1]                   # (one tap on one sample does not leave int16)
    assert np.all(want[0][0, :L] == 32767) and np.all(want[0][1, :L] == -32768) and np.all(want[0][2, :L] == -32768)


@pytest.mark.parametrize("form", FORMS)
def test_a_unit_impulse_response_gives_what_the_checker_says(form):
    rng = np.random.default_rng(3)
    clip = rng.integers(-32768, 32768, 700).astype(np.int16)
    clip[:6] = [32767, -32768, -1, 0, 1, 32766]
    st = _Setup([clip], [np.array([16384], np.int16), np.array([RC.TAP_MAX], np.int16)])
    L = 300
    plan, rplan = _plan([(0, 0), (0, 0), (0, 450)]), RC.make_reverb_plan([0, 1, 0])
    st.check(plan, rplan, L, L, form)
    got = st.run(plan, rplan, L, L, form)[0]
    x = clip.astype(np.int64)
    assert np.array_equal(got[0], ((x[:L] + 1) >> 1).astype(np.int16))       # h = [16384]: half the sample, rounded half up
    assert np.array_equal(got[1], ((x[:L] * RC.TAP_MAX + 16384) >> 15).astype(np.int16))
    assert np.array_equal(got[2, :250], ((x[450:] + 1) >> 1).astype(np.int16)) and not got[2, 250:].any()


@pytest.mark.parametrize("form", FORMS)
def test_plan_entries_outside_their_tables_are_clamped(form):
    st, _ = _case(65)
    L = 300
    plan = _plan([(99, 5), (-5, 70), (1, -4), (1, 2 ** 31 - 1), (2, 3)])
    rplan = RC.make_reverb_plan([99, 0, -7, 1, 2 ** 31 - 1])
    rec = st.check(plan, rplan, L, L, form)                                   # (the checker clamps as the contract says)
    assert rec["rir"].tolist() == [2, 0, -1, 1, 2]


def test_speech_behind_the_2_31st_sample_of_its_corpus():
    """A clip behind the 2^31-th sample of a 4.3 GB buffer (uninitialised, never read elsewhere): a 32-bit index would
    read the buffer's start."""
    import torch
    from gtcrn_micro_amd.data import Corpus
    st, _ = _case(65)
    base = (1 << 31) + 1
    n = st.spcm.size
    pcm = torch.empty((1 << 31) + n + 64, device="cuda", dtype=torch.int16)
    pcm[base:base + n] = torch.from_numpy(st.spcm).cuda()
    far = Corpus.from_tensors(pcm, torch.from_numpy(st.soff + base).cuda())
    plan, rplan = _plan([(1, 64), (0, 0), (1, 4000)]), RC.make_reverb_plan([0, 1, -1])
    for form in FORMS:
        st.check(plan, rplan, 300, 300, form, sp=far)
    del pcm, far
    torch.cuda.empty_cache()


@pytest.mark.parametrize("B", [255, 256])
def test_the_block_the_library_chooses_changes_at_256_workgroups(B):
    """form 0 / 2: the large block once B rows of it make 256 workgroups.  Either side of that, against the checker."""
    st, _ = _case(65)
    L = 300
    rng = np.random.default_rng(B)
    plan = _plan([(1, int(s)) for s in rng.integers(0, 4000, B)])
    rplan = RC.make_reverb_plan(rng.integers(-1, 3, B))
    want = st.want(plan, rplan, L, L)
    for form in (0, 2):
        st.check(plan, rplan, L, L, form, want)


# ---- BatchSource(rirs=) ------------------------------------------------------------------------------------------------------
def _corpora(seed=21):
    from gtcrn_micro_amd.data import Corpus, RirBank
    rng = np.random.default_rng(seed)
    speech = [rng.integers(-9000, 9000, n).astype(np.int16) for n in (9000, 5, 20000, 4099, 6001)]
    noise = [rng.integers(-3000, 3000, n).astype(np.int16) for n in (100, 7000, 3)]
    rirs = []
    for K in (1, 40, 700, 3000):
        h = rng.standard_normal(K) * np.exp(-np.arange(K) / (0.2 * K + 1))
        h[0] = 1.0
        rirs.append(h)
    bank = RirBank.from_arrays(rirs, normalize="peak", trim_direct=True)
    return speech, noise, Corpus.from_arrays(speech), Corpus.from_arrays(noise), bank


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def test_p_reverb_0_is_the_source_without_a_bank_bit_for_bit():
    import torch
    from gtcrn_micro_amd.data import BatchSource
    _, _, sp, nz, bank = _corpora()
    B, L = 6, 4099
    a = BatchSource(sp, noise=nz, B=B, L=L, seed=5)
    b = BatchSource(sp, noise=nz, B=B, L=L, seed=5, rirs=bank, p_reverb=0.0)
    for _ in range(2):
        (an, ac), (bn, bc) = a.draw(), b.draw()
        torch.cuda.synchronize()
        assert torch.equal(an.view(torch.int32), bn.view(torch.int32)) and torch.equal(ac.view(torch.int32), bc.view(torch.int32))
        assert torch.equal(a.plan, b.plan) and torch.equal(a.records, b.records)
        assert np.all(b.reverb_plan_numpy()["rir"] == -1) and not b.reverb_records_numpy()["saturated"].any()
    assert a.step() == b.step() == 2


@pytest.mark.parametrize("p", [1.0, 0.5])
@pytest.mark.parametrize("form", [0, 1, 4])
def test_full_draw_equals_the_reverb_checker_fed_into_the_batch_checker(p, form):
    import torch
    from gtcrn_micro_amd.data import BatchSource
    speech, noise, sp, nz, bank = _corpora()
    B, L, seed, item0 = 12, 4099, 0x5eed, 24
    src = BatchSource(sp, noise=nz, B=B, L=L, seed=seed, item0=item0, rirs=bank, p_reverb=p, reverb_form=form)
    soff, noff = sp.offsets.cpu().numpy(), nz.offsets.cpu().numpy()
    taps, roff = bank.taps.cpu().numpy(), bank.offsets.cpu().numpy()
    for step in range(2):
        noisy, clean = src.draw()
        torch.cuda.synchronize()
        plan, rplan = src.plan_numpy(), src.reverb_plan_numpy()
        BC.assert_same_plan(plan, BC.plan(soff, noff, B, L, seed, step, item0=item0))
        assert rplan.tobytes() == RC.reverb_plan(bank.n, p, B, seed, step, item0=item0).tobytes()
        wet = int((rplan["rir"] >= 0).sum())
        assert wet == B if p == 1.0 else 0 < wet < B
        ws, wo, wp, wr = RC.reverb(np.concatenate(speech), soff, taps, roff, plan, rplan, L, src.staged_stride)
        assert src.reverb_records_numpy().tobytes() == wr.tobytes()
        assert np.array_equal(src.staged.cpu().numpy().reshape(B, -1)[:, :L], ws[:, :L])
        assert np.array_equal(src.staged_offsets.cpu().numpy(), wo)
        assert src.staged_plan.cpu().numpy().tobytes() == wp.tobytes()
        wn, wc, wrec = BC.mix(ws.reshape(-1), wo, np.concatenate(noise), noff, wp, L)
        assert src.records.cpu().numpy().tobytes() == wrec.tobytes()
        assert np.array_equal(_bits(noisy), wn.view(np.int32)) and np.array_equal(_bits(clean), wc.view(np.int32))
    assert src.step() == 2
    # a caller-written reverb plan, with the batch plan drawn: the step moves on, the bank is not consulted for row 0
    mine = RC.make_reverb_plan([-1, 3] * (B // 2))
    from gtcrn_micro_amd.data import reverb_plan_to_device
    src.draw(reverb_plan=reverb_plan_to_device(mine, "cuda"))
    assert src.reverb_records_numpy()["rir"].tolist() == [-1, 3] * (B // 2) and src.step() == 3


def test_a_captured_draw_with_reverb_replays_consecutive_batches():
    import torch
    from gtcrn_micro_amd.data import BatchSource
    _, _, sp, nz, bank = _corpora()
    B, L = 6, 4099
    eager = BatchSource(sp, noise=nz, B=B, L=L, seed=5, rirs=bank, p_reverb=0.5)
    want = []
    for _ in range(3):
        n, c = eager.draw()
        want.append((n.clone(), c.clone(), eager.plan.clone(), eager.records.clone(), eager.reverb_plan.clone(),
                     eager.reverb_records.clone()))
    src = BatchSource(sp, noise=nz, B=B, L=L, seed=5, rirs=bank, p_reverb=0.5)
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
        for got, ref in zip((out[0], out[1], src.plan, src.records, src.reverb_plan, src.reverb_records), want[k]):
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), k
    assert src.step() == 3 and eager.step() == 3
    assert not torch.equal(want[0][4], want[1][4]) or not torch.equal(want[1][4], want[2][4])
    assert not torch.equal(want[0][0], want[1][0])


def test_bad_arguments_are_refused():
    import torch
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd._lib import lib
    from gtcrn_micro_amd.data import BatchSource, Corpus, RirBank
    speech, _, sp, nz, bank = _corpora()
    with pytest.raises(GtcrnError):
        BatchSource(sp, paired_clean=Corpus.from_arrays(speech), B=2, L=100, rirs=bank, p_reverb=0.5)
    with pytest.raises(GtcrnError):
        BatchSource(sp, noise=nz, B=2, L=100, rirs=bank, p_reverb=1.5)
    with pytest.raises(GtcrnError):
        BatchSource(sp, noise=nz, B=2, L=100, p_reverb=0.5)
    with pytest.raises(GtcrnError):
        BatchSource(sp, noise=nz, B=2, L=100, rirs="bank")
    with pytest.raises(GtcrnError):
        RirBank.from_tensors(torch.full((4,), 32640, dtype=torch.int16, device="cuda"), torch.tensor([0, 4], device="cuda"))
    with pytest.raises(GtcrnError):
        RirBank.from_tensors(torch.zeros(16385, dtype=torch.int16, device="cuda"), torch.tensor([0, 16385], device="cuda"))
    src = BatchSource(sp, noise=nz, B=2, L=100, rirs=bank, p_reverb=0.5)
    with pytest.raises(GtcrnError):
        src.draw(reverb_plan=torch.zeros((3, 2), dtype=torch.int32, device="cuda"))
    with pytest.raises(GtcrnError):
        BatchSource(sp, noise=nz, B=2, L=100).draw(reverb_plan=torch.zeros((2, 2), dtype=torch.int32, device="cuda"))
    # the C entry point on real device buffers: refused before anything is enqueued
    args = [sp.pcm.data_ptr(), sp.offsets.data_ptr(), sp.n, bank.taps.data_ptr(), bank.offsets.data_ptr(), bank.n, bank.table.data_ptr(),
            bank.table.numel(), src.plan.data_ptr(), src.reverb_plan.data_ptr(), 2, 100, src.staged.data_ptr(), src.staged_stride,
            src.staged_offsets.data_ptr(), src.staged_plan.data_ptr(), src.reverb_records.data_ptr(), src._rws.data_ptr(), 0, None]
    for pos, val in ((10, 0), (11, 0), (13, 99), (18, 5), (6, None), (12, None), (5, 0)):
        bad = list(args)
        bad[pos] = val
        assert lib().gtcrn_batch_reverb(*bad) == -1, (pos, val)
    assert lib().gtcrn_batch_reverb(*args) == 0
    torch.cuda.synchronize()


def test_bank_round_trips_through_wav_files_and_the_npy_pair(tmp_path):
    import torch
    from gtcrn_micro_amd.data import RirBank, quantize_rirs
    from gtcrn_micro_amd.infer import write_wav_pcm16
    rng = np.random.default_rng(2)
    hs = [np.r_[np.zeros(30), rng.standard_normal(n) * np.exp(-np.arange(n) / 50.0)] for n in (1, 200, 1601)]
    for h in hs:
        h[30] = 4.0
    a = RirBank.from_arrays(hs)
    assert a.n == 3 and a.offsets.cpu().tolist() == [0, 1, 201, 1802]        # the 30 leading taps are gone
    assert a.taps.cpu().numpy()[[0, 1, 201]].tolist() == [RC.TAP_MAX] * 3
    a.save(str(tmp_path / "bank"))
    b = RirBank.load(str(tmp_path / "bank"))
    assert torch.equal(a.taps, b.taps) and torch.equal(a.offsets, b.offsets) and torch.equal(a.table, b.table)
    paths = []
    for k, q in enumerate(quantize_rirs(hs)):
        paths.append(str(tmp_path / f"rir{k}.wav"))
        write_wav_pcm16(paths[-1], q.astype(np.float32) / 32768.0)
    c = RirBank.from_wavs(paths)
    assert torch.equal(c.offsets, a.offsets) and torch.equal(c.taps, a.taps)


def test_matrix_form_uses_no_scratch():
    """From the committed resource dump of csrc/reverb.hip (profiles/reverb_resources.txt)."""
    rows = [l for l in open(os.path.join(ROOT, "profiles", "reverb_resources.txt")) if "k_reverb_mfma" in l and not l.startswith("#")]
    assert len(rows) == 2, "one row per block size of the matrix-form kernel"
    for l in rows:
        assert "ScratchSize [bytes/lane]: 0 " in l and "VGPRs Spill: 0 " in l, l
