"""GPU tests of "dereverberation targets: early or direct clean" (csrc/reverb.hip and csrc/batch.hip through
gtcrn_micro_amd.data): every form of gtcrn_batch_reverb_split against the numpy statement of the contract
(tests/target_checker.py) BIT FOR BIT -- both staged rows, guard words, offsets, rewritten plan and 32-byte records -- around
the split, the 256-tap seam block, the 64-tap chunk and the 2048- and 8192-sample blocks; the same outputs against the existing
entry points on the device; gtcrn_batch_mix_target against gtcrn_batch_mix and the checker; BatchSource with target_ms= and
target=.  The contract is exact: nothing below has a tolerance except the 1 ulp on the batch plan's two pow results that
tests/test_gpu_batch.py allows as well."""
import os

import numpy as np
import pytest

from conftest import ROOT

import __graft_entry__ as graft
import batch_checker as BC
import reverb_checker as RC
import target_checker as TC

pytestmark = pytest.mark.gpu
BLOCK, BIG_BLOCK = 2048, 8192      # gtr::BLOCK, gtr::BIG_BLOCK: output samples of one workgroup
FORMS = [1, 3, 4]                  # plain; matrix with the small and with the large block (form 2 is one of these by the shape)
GUARD = 0x5A5A
KS = [1, 17, 256, 257, 700, 16384]
LS = [1, 17, 255, BLOCK - 1, BLOCK + 1]
LS_BIG = [BIG_BLOCK - 1, BIG_BLOCK + 1]        # form 4 only: a whole large block (its 8-byte store path) and the one behind it


def _splits(K):
    return sorted({E for E in (1, 16, 255, 256, 257, K - 1, K) if 1 <= E <= K})


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


class _Setup:
    """Corpus, bank and split on the device, with their host copies."""

    def __init__(self, speech, rirs, split):
        from gtcrn_micro_amd.data import Corpus, RirBank
        self.speech, self.rirs = speech, rirs
        self.sp = Corpus.from_arrays(speech)
        self.bank = RirBank.from_arrays(rirs, trim_direct=False)
        self.spcm, self.soff = np.concatenate(speech), self.sp.offsets.cpu().numpy()
        self.taps, self.roff = np.concatenate(rirs), self.bank.offsets.cpu().numpy()
        self.set_split(split)

    def set_split(self, split, table_of=None):
        """split: what d_split holds, as given (the library clamps it); table_of: the split the table is prepared from."""
        import torch
        self.split = np.asarray(split, np.int32)
        self.d_split = torch.from_numpy(self.split).cuda()
        _, self.table = self.bank.split_table(self.split if table_of is None else table_of)

    def want(self, plan, rplan, L, stride):
        return TC.split(self.spcm, self.soff, self.taps, self.roff, self.split, plan, rplan, L, stride)

    def run(self, plan, rplan, L, stride, form, sp=None):
        """gtcrn_batch_reverb_split on guarded buffers -> (wet, target (B, stride), offsets, staged plan, records), all numpy."""
        import torch
        from gtcrn_micro_amd._lib import _check, lib
        from gtcrn_micro_amd.data import plan_to_device, reverb_plan_to_device, reverb_split_workspace_bytes
        sp = sp or self.sp
        B = len(plan)
        wet = torch.full((B * stride + 64,), GUARD, device="cuda", dtype=torch.int16)
        tgt = torch.full((B * stride + 64,), GUARD, device="cuda", dtype=torch.int16)
        so = torch.full((B + 3,), -7, device="cuda", dtype=torch.int64)
        splan = torch.full((B + 1, 8), -3, device="cuda", dtype=torch.int32)
        rec = torch.full((B + 1, 8), -9, device="cuda", dtype=torch.int32)
        nws = reverb_split_workspace_bytes(B, L)
        ws = torch.full((nws + 256,), 0xA5, device="cuda", dtype=torch.uint8)
        p, rp = plan_to_device(plan, "cuda"), reverb_plan_to_device(rplan, "cuda")
        bk = self.bank
        _check(lib().gtcrn_batch_reverb_split(
            sp.pcm.data_ptr(), sp.offsets.data_ptr(), sp.n, bk.taps.data_ptr(), bk.offsets.data_ptr(), self.d_split.data_ptr(), bk.n,
            self.table.data_ptr() if form != 1 else None, self.table.numel(), p.data_ptr(), rp.data_ptr(), B, L, wet.data_ptr(),
            tgt.data_ptr(), stride, so.data_ptr(), splan.data_ptr(), rec.data_ptr(), ws.data_ptr(), form, None))
        torch.cuda.synchronize()
        assert bool((wet[B * stride:] == GUARD).all()) and bool((tgt[B * stride:] == GUARD).all()), "wrote behind a staged corpus"
        assert bool((so[B + 1:] == -7).all()) and bool((splan[B:] == -3).all()) and bool((rec[B:] == -9).all())
        assert bool((ws[nws:] == 0xA5).all()), "wrote past gtcrn_batch_reverb_split_workspace_bytes"
        return (wet[:B * stride].cpu().numpy().reshape(B, stride), tgt[:B * stride].cpu().numpy().reshape(B, stride),
                so[:B + 1].cpu().numpy(), splan[:B].cpu().numpy().view(BC.PLAN_DTYPE).reshape(B),
                rec[:B].cpu().numpy().view(TC.SPLIT_RECORD_DTYPE).reshape(B))

    def check(self, plan, rplan, L, stride, form, want=None, sp=None):
        ww, wt, wo, wp, wr = want or self.want(plan, rplan, L, stride)
        gw, gt, go, gp, gr = self.run(plan, rplan, L, stride, form, sp)
        assert gr.tobytes() == wr.tobytes(), (gr, wr)
        for name, g, w in (("wet", gw, ww), ("target", gt, wt)):
            bad = np.argwhere(g[:, :L] != w[:, :L])
            assert bad.size == 0, (name, len(bad), bad[:5], g[:, :L][tuple(bad[0])], w[:, :L][tuple(bad[0])])
            assert np.all(g[:, L:] == GUARD), f"the tail of a staged {name} row was touched"
        assert np.array_equal(go, wo) and gp.tobytes() == wp.tobytes()
        return wr


def _plan(rows):
    """rows of (sclip, sstart): the other fields of a batch item only pass through the convolution."""
    return BC.make_plan([(c, s, 3 + b, 11 * b, 0.25 + b, 0.05 * (b + 1)) for b, (c, s) in enumerate(rows)])


_cases = {}


def _case(K):
    """The set-up of one K -- one response per split of _splits(K), all of the same taps, and a three-tap one split at 2 -- and,
    once computed, its expected results (shared by the forms)."""
    if K not in _cases:
        rng = np.random.default_rng(200 + K)
        n = 2 * K + 4200
        long_ = rng.integers(-32768, 32768, n).astype(np.int16)
        long_[K:K + 4] = [32767, -32768, 32767, -32768]
        speech = [rng.integers(-32768, 32768, 9).astype(np.int16), long_, rng.integers(-32768, 32768, max(1, K // 2)).astype(np.int16)]
        h = (rng.integers(-RC.TAP_MAX, RC.TAP_MAX + 1, K) // (1 if K < 300 else 8)).astype(np.int16)
        h[0], h[-1] = RC.TAP_MAX, -RC.TAP_MAX if K > 1 else RC.TAP_MAX
        Es = _splits(K)
        _cases[K] = (_Setup(speech, [h] * len(Es) + [np.array([20000, -9000, 4000], np.int16)], Es + [2]), {})
    return _cases[K]


def _batches(K, L, k):
    """k: a counter that rotates the responses (and with them the splits) through the rows."""
    Es = _splits(K)
    nE, n = len(Es), 2 * K + 4200
    odd = L + 5 if (L + 5) % 4 else L + 6
    r = [(k + i) % nE for i in range(5)]
    E = [Es[i] for i in r]
    return [
        # one clip; starts 0 and 1 (zeros before the clip), E - 1 and E (the early taps' history just inside the clip) and K
        (_plan([(1, 0), (1, 1), (1, E[2] - 1), (1, E[3]), (1, K)]), RC.make_reverb_plan(r), (L + 3) // 4 * 4),
        # a clip shorter than the window (and mostly than E and K), dry rows between wet ones, a clip of K / 2 samples, a window that
        # leaves its clip, two rows sharing a response, under a stride above L that rules 8-byte stores out
        (_plan([(0, 0), (1, 7), (2, 0), (1, n - 3), (1, n - 2)]), RC.make_reverb_plan([r[0], -1, r[1], -1, r[0]]), odd),
        (_plan([(1, K + 2)]), RC.make_reverb_plan([r[4]]), L),
    ]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("K", KS)
def test_every_form_equals_the_checker_bit_for_bit(K, form):
    st, wants = _case(K)
    Es = _splits(K)
    clamped, seen = 0, set()
    for li, L in enumerate(LS + (LS_BIG if form == 4 else [])):
        for k, (plan, rplan, stride) in enumerate(_batches(K, L, 2 * li)):
            if (L > BLOCK - 2 and K > 1000 and k != 2) or (L > BIG_BLOCK - 2 and k == 1):
                continue                                 # (the blocks' edges at 16384 taps: the one-row batch)
            if (L, k) not in wants:
                wants[(L, k)] = st.want(plan, rplan, L, stride)
            rec = st.check(plan, rplan, L, stride, form, wants[(L, k)])
            clamped += int(rec["saturated"].sum()) + int(rec["target_saturated"].sum())
            wet = rplan["rir"] >= 0
            assert np.array_equal(rec["ntaps"], np.where(wet, K, 0))
            assert np.array_equal(rec["split"], np.where(wet, np.array(Es + [2])[np.maximum(rplan["rir"], 0)], 0))
            seen |= set(rec["split"][wet].tolist())
    assert seen == set(Es), "a split was never drawn"
    assert clamped > 0 or K == 1, "no case clamped a sample"


@pytest.mark.parametrize("form", FORMS)
def test_extreme_speech_against_extreme_taps_split_in_the_middle(form):
    """The largest digit sums on both sides of the seam: speech all 32767 / all -32768 against 16384 taps all at the bank's
    maximum / minimum, split at 8191 and 8192."""
    K, L = RC.MAX_TAPS, 300
    if "extreme" not in _cases:
        speech = [np.full(K + L, 32767, np.int16), np.full(K + L, -32768, np.int16)]
        st = _Setup(speech, [np.full(K, RC.TAP_MAX, np.int16), np.full(K, -RC.TAP_MAX, np.int16)], [8191, 8192])
        plan, rplan = _plan([(0, K), (0, K), (1, K), (1, K), (1, 0)]), RC.make_reverb_plan([0, 1, 0, 1, 0])
        _cases["extreme"] = (st, plan, rplan, st.want(plan, rplan, L, L + 3))
    st, plan, rplan, want = _cases["extreme"]
    rec = st.check(plan, rplan, L, L + 3, form, want)
    assert rec["saturated"].tolist() == [L, L, L, L, L - 1] and rec["target_saturated"].tolist() == [L, L, L, L, L - 1]
    assert rec["split"].tolist() == [8191, 8192, 8191, 8192, 8191]


@pytest.mark.parametrize("form", FORMS)
def test_splits_and_plan_entries_outside_their_ranges_are_clamped(form):
    rng = np.random.default_rng(9)
    clip = rng.integers(-20000, 20000, 3000).astype(np.int16)
    hs = [(rng.integers(-RC.TAP_MAX, RC.TAP_MAX + 1, K) // 4).astype(np.int16) for K in (257, 40, 300)]
    st = _Setup([clip[:50], clip, clip[:700]], hs, [0, 99999, -(2 ** 31)])
    L = 300
    plan = _plan([(99, 5), (-5, 70), (1, -4), (1, 2 ** 31 - 1), (2, 3), (1, 600)])
    rplan = RC.make_reverb_plan([99, 0, -7, 1, 2 ** 31 - 1, 1])
    rec = st.check(plan, rplan, L, L, form)                                   # (the checker clamps as the contract says)
    assert rec["rir"].tolist() == [2, 0, -1, 1, 2, 1] and rec["split"].tolist() == [1, 1, 0, 40, 1, 40]


def test_a_table_of_another_split_moves_the_target_of_the_matrix_form_only():
    """The matrix form takes E from the table's header, the plain form and the record from d_split: with a table prepared
    from another split the wet rows are what they were, the target is the table's, and nothing is read out of range."""
    st, _ = _case(700)
    Es = _splits(700)
    other = [Es[(i + 2) % len(Es)] for i in range(len(Es))] + [3]
    L = 300
    plan, rplan = _plan([(1, 800), (1, 5), (0, 0), (1, 1500)]), RC.make_reverb_plan([0, 3, 5, 7])
    ww, _, wo, wp, wr = st.want(plan, rplan, L, L)
    st.set_split(Es + [2], table_of=other)
    try:
        for form in (3, 4):
            gw, gt, go, gp, gr = st.run(plan, rplan, L, L, form)
            assert np.array_equal(gw, ww) and np.array_equal(go, wo) and gp.tobytes() == wp.tobytes()
            assert np.array_equal(gr["split"], wr["split"]) and np.array_equal(gr["saturated"], wr["saturated"])
            wt = TC.split(st.spcm, st.soff, st.taps, st.roff, other, plan, rplan, L, L)[1]
            assert np.array_equal(gt, wt)
        # a table cut short of the last response's groups: that response's row stays dry in both outputs, the others do not move
        st.table = st.table[:-512].clone()
        gw, gt, _, _, _ = st.run(plan, rplan, L, L, 3)
        dry = TC.split(st.spcm, st.soff, st.taps, st.roff, other, plan, RC.make_reverb_plan([0, 3, 5, -1]), L, L)
        assert np.array_equal(gw, dry[0]) and np.array_equal(gt, dry[1]) and not np.array_equal(gw[3], ww[3])
    finally:
        st.set_split(Es + [2])


@pytest.mark.parametrize("B", [255, 256])
def test_the_block_the_library_chooses_changes_at_256_workgroups(B):
    """form 0 / 2: the large block once B rows of it make 256 workgroups.  Either side of that, against the checker."""
    st, _ = _case(257)
    L = 300
    rng = np.random.default_rng(B)
    plan = _plan([(1, int(s)) for s in rng.integers(0, 4000, B)])
    rplan = RC.make_reverb_plan(rng.integers(-1, len(_splits(257)) + 1, B))
    want = st.want(plan, rplan, L, L)
    for form in (0, 2):
        st.check(plan, rplan, L, L, form, want)


def test_speech_behind_the_2_31st_sample_of_its_corpus():
    """A clip behind the 2^31-th sample of a 4.3 GB buffer (uninitialised, never read elsewhere): a 32-bit index would read
    the buffer's start."""
    import torch
    from gtcrn_micro_amd.data import Corpus
    st, _ = _case(257)
    base = (1 << 31) + 1
    n = st.spcm.size
    pcm = torch.empty((1 << 31) + n + 64, device="cuda", dtype=torch.int16)
    pcm[base:base + n] = torch.from_numpy(st.spcm).cuda()
    far = Corpus.from_tensors(pcm, torch.from_numpy(st.soff + base).cuda())
    plan, rplan = _plan([(1, 256), (0, 0), (1, 4000)]), RC.make_reverb_plan([2, 4, -1])
    want = st.want(plan, rplan, 300, 300)
    for form in FORMS:
        st.check(plan, rplan, 300, 300, form, want, sp=far)
    del pcm, far
    torch.cuda.empty_cache()


# ---- the same outputs from the existing entry points, on the device ------------------------------------------------------------
def _reverb(sp, bank, plan, rplan, L, stride, form=0):
    """gtcrn_batch_reverb -> (staged (B, stride) int16 tensor, staged plan tensor, records tensor)."""
    import torch
    from gtcrn_micro_amd._lib import _check, lib
    from gtcrn_micro_amd.data import plan_to_device, reverb_plan_to_device, reverb_workspace_bytes
    B = len(plan)
    staged = torch.zeros(B * stride, device="cuda", dtype=torch.int16)
    so = torch.zeros(B + 1, device="cuda", dtype=torch.int64)
    splan = torch.zeros((B, 8), device="cuda", dtype=torch.int32)
    rec = torch.zeros((B, 4), device="cuda", dtype=torch.int32)
    ws = torch.empty(reverb_workspace_bytes(B, L), device="cuda", dtype=torch.uint8)
    p, rp = plan_to_device(plan, "cuda"), reverb_plan_to_device(rplan, "cuda")
    _check(lib().gtcrn_batch_reverb(sp.pcm.data_ptr(), sp.offsets.data_ptr(), sp.n, bank.taps.data_ptr(), bank.offsets.data_ptr(), bank.n,
                                    bank.table.data_ptr(), bank.table.numel(), p.data_ptr(), rp.data_ptr(), B, L, staged.data_ptr(),
                                    stride, so.data_ptr(), splan.data_ptr(), rec.data_ptr(), ws.data_ptr(), form, None))
    torch.cuda.synchronize()
    return staged.cpu().numpy().reshape(B, stride), splan.cpu().numpy(), rec.cpu().numpy()


@pytest.mark.parametrize("form", [0, 1, 3, 4])
def test_wet_is_the_existing_call_and_target_is_the_existing_call_on_the_truncated_bank(form):
    from gtcrn_micro_amd.data import RirBank
    st, _ = _case(700)
    Es = _splits(700) + [2]
    L, stride = 2049, 2052
    rng = np.random.default_rng(form)
    plan = _plan([(1, int(s)) for s in rng.integers(0, 3000, 9)])
    rplan = RC.make_reverb_plan([0, 1, 2, -1, 3, 4, 5, 6, 7])
    gw, gt, _, gp, gr = st.run(plan, rplan, L, stride, form)
    ew, ep, er = _reverb(st.sp, st.bank, plan, rplan, L, stride)             # (a) any split: the wet rows are today's
    assert np.array_equal(gw[:, :L], ew[:, :L]) and gp.view(np.int32).reshape(9, 8).tolist() == ep.tolist()
    assert gr["rir"].tolist() == er[:, 0].tolist() and gr["ntaps"].tolist() == er[:, 1].tolist()
    assert gr["saturated"].tolist() == er[:, 2].tolist()
    cut = RirBank.from_arrays([h[:E] for h, E in zip(st.rirs, Es)], trim_direct=False)
    tw, _, tr = _reverb(st.sp, cut, plan, rplan, L, stride)                  # (b) the target: today's call on the truncated bank
    assert np.array_equal(gt[:, :L], tw[:, :L]) and gr["target_saturated"].tolist() == tr[:, 2].tolist()
    assert gr["split"].tolist() == tr[:, 1].tolist()


@pytest.mark.parametrize("form", [1, 3, 4])
def test_a_split_at_the_last_tap_gives_the_existing_call_twice(form):
    st, _ = _case(700)
    L = 300
    plan, rplan = _plan([(1, 900), (1, 3), (2, 0), (0, 2)]), RC.make_reverb_plan([0, 7, -1, 3])
    st.set_split([1 << 30] * 8)                                              # (c) E_r = K_r everywhere
    try:
        gw, gt, _, _, gr = st.run(plan, rplan, L, L, form)
    finally:
        st.set_split(_splits(700) + [2])
    ew, _, er = _reverb(st.sp, st.bank, plan, rplan, L, L)
    assert np.array_equal(gw, ew) and np.array_equal(gt, ew)
    assert gr["split"].tolist() == [700, 3, 0, 700] and gr["target_saturated"].tolist() == gr["saturated"].tolist() == er[:, 2].tolist()


# ---- gtcrn_batch_mix_target ------------------------------------------------------------------------------------------------------
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


def _mix(sp, nz, target, plan, B, L, stride=None):
    """gtcrn_batch_mix (target None) or gtcrn_batch_mix_target on guarded rows -> (noisy, clean, records) tensors."""
    import torch
    from gtcrn_micro_amd._lib import _check, lib
    from gtcrn_micro_amd.data import workspace_bytes
    stride = stride or L
    noisy = torch.full((B * stride + 16,), 7.0, device="cuda")
    clean = torch.full((B * stride + 16,), 7.0, device="cuda")
    rec = torch.zeros((B, 10), device="cuda", dtype=torch.int32)
    ws = torch.empty(workspace_bytes(B, L), device="cuda", dtype=torch.uint8)
    head = [sp.pcm.data_ptr(), sp.offsets.data_ptr(), sp.n, nz.pcm.data_ptr(), nz.offsets.data_ptr(), nz.n]
    tail = [plan.data_ptr(), B, L, noisy.data_ptr(), stride, clean.data_ptr(), stride, rec.data_ptr(), ws.data_ptr(), 7, None]
    if target is None:
        _check(lib().gtcrn_batch_mix(*head, *tail))
    else:
        _check(lib().gtcrn_batch_mix_target(*head, target.data_ptr(), *tail))
    torch.cuda.synchronize()
    for t in (noisy, clean):
        rows = t[:B * stride].view(B, stride)
        assert bool((rows[:, L:] == 7.0).all()) and bool((t[B * stride:] == 7.0).all()), "wrote outside a row"
    return noisy[:B * stride].view(B, stride)[:, :L], clean[:B * stride].view(B, stride)[:, :L], rec


@pytest.mark.parametrize("L,stride", [(1, 1), (17, 20), (2047, 2047), (4099, 4100), (9001, 9004)])
def test_mix_target_with_the_speech_as_its_own_target_is_the_mix_and_with_a_target_the_checker(L, stride):
    import torch
    from gtcrn_micro_amd.data import Corpus, plan_to_device
    speech, noise, sp, nz, _ = _corpora()
    rng = np.random.default_rng(L)
    target = [rng.integers(-32768, 32768, len(s)).astype(np.int16) for s in speech]
    tg = Corpus.from_arrays(target)
    B = 5
    soff, noff = sp.offsets.cpu().numpy(), nz.offsets.cpu().numpy()
    plan = BC.plan(soff, noff, B, L, 77, 3)
    plan["sclip"][:3] = [1, 3, 0]                        # the 5-sample clip; windows that leave their clips
    plan["sstart"][:3] = [2, 4000, 8990]
    p = plan_to_device(plan, "cuda")
    an, ac, ar = _mix(sp, nz, None, p, B, L, stride)
    bn, bc, br = _mix(sp, nz, sp.pcm, p, B, L, stride)                       # (d)
    assert torch.equal(an.view(torch.int32), bn.view(torch.int32)) and torch.equal(ac.view(torch.int32), bc.view(torch.int32))
    assert torch.equal(ar, br)
    tn, tc, tr = _mix(sp, nz, tg.pcm, p, B, L, stride)
    wn, wc, wr = TC.mix_target(np.concatenate(speech), soff, np.concatenate(noise), noff, np.concatenate(target), plan, L)
    assert tr.cpu().numpy().tobytes() == wr.tobytes()
    assert np.array_equal(_bits(tn), wn.view(np.int32)) and np.array_equal(_bits(tc), wc.view(np.int32))
    assert torch.equal(tn.view(torch.int32), an.view(torch.int32))            # noisy does not look at the target


# ---- BatchSource(target_ms=), BatchSource(target=) -------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1.0, 0.5])
@pytest.mark.parametrize("ms", [0, 2.5, 50])
def test_full_draw_equals_the_split_checker_fed_into_the_target_mix_checker(ms, p):
    import torch
    from gtcrn_micro_amd.data import BatchSource
    speech, noise, sp, nz, bank = _corpora()
    B, L, seed, item0 = 12, 4099, 0x5eed, 24
    src = BatchSource(sp, noise=nz, B=B, L=L, seed=seed, item0=item0, rirs=bank, p_reverb=p, target_ms=ms,
                      reverb_form=0 if ms != 2.5 else 1)
    soff, noff = sp.offsets.cpu().numpy(), nz.offsets.cpu().numpy()
    taps, roff = bank.taps.cpu().numpy(), bank.offsets.cpu().numpy()
    split = bank.split_for(ms)
    assert split.tolist() == np.minimum(np.diff(roff), 1 + int(16 * ms)).tolist() and split[0] == 1      # (trimmed: the direct path is tap 0)
    assert np.array_equal(split, TC.split_for([taps[int(roff[r]):int(roff[r + 1])] for r in range(bank.n)], ms))
    assert np.array_equal(src.split.cpu().numpy(), split)
    for step in range(2):
        noisy, clean = src.draw()
        torch.cuda.synchronize()
        plan, rplan = src.plan_numpy(), src.reverb_plan_numpy()
        BC.assert_same_plan(plan, BC.plan(soff, noff, B, L, seed, step, item0=item0))
        assert rplan.tobytes() == RC.reverb_plan(bank.n, p, B, seed, step, item0=item0).tobytes()
        ww, wt, wo, wp, wr = TC.split(np.concatenate(speech), soff, taps, roff, split, plan, rplan, L, src.staged_stride)
        assert src.split_records_numpy().tobytes() == wr.tobytes()
        assert np.array_equal(src.staged.cpu().numpy().reshape(B, -1)[:, :L], ww[:, :L])
        assert np.array_equal(src.staged_target.cpu().numpy().reshape(B, -1)[:, :L], wt[:, :L])
        assert np.array_equal(src.staged_offsets.cpu().numpy(), wo) and src.staged_plan.cpu().numpy().tobytes() == wp.tobytes()
        wn, wc, wrec = TC.mix_target(ww.reshape(-1), wo, np.concatenate(noise), noff, wt.reshape(-1), wp, L)
        assert src.records.cpu().numpy().tobytes() == wrec.tobytes()
        assert np.array_equal(_bits(noisy), wn.view(np.int32)) and np.array_equal(_bits(clean), wc.view(np.int32))
        wet = rplan["rir"] >= 2                          # (the long responses: longer than any of these targets)
        assert not wet.any() or not np.array_equal(wt[wet], ww[wet]), "no target differs from its wet row"
    assert src.step() == 2


def test_a_target_longer_than_every_response_draws_what_the_source_without_a_target_draws():
    import torch
    from gtcrn_micro_amd.data import BatchSource
    _, _, sp, nz, bank = _corpora()
    B, L = 6, 4099
    a = BatchSource(sp, noise=nz, B=B, L=L, seed=5, item0=6, rirs=bank, p_reverb=0.5)
    b = BatchSource(sp, noise=nz, B=B, L=L, seed=5, item0=6, rirs=bank, p_reverb=0.5, target_ms=2000)
    assert b.split.cpu().tolist() == np.diff(bank.offsets.cpu().numpy()).tolist()
    for _ in range(2):
        (an, ac), (bn, bc) = a.draw(), b.draw()
        torch.cuda.synchronize()
        assert torch.equal(an.view(torch.int32), bn.view(torch.int32)) and torch.equal(ac.view(torch.int32), bc.view(torch.int32))
        assert torch.equal(a.plan, b.plan) and torch.equal(a.records, b.records) and torch.equal(a.reverb_plan, b.reverb_plan)
        assert torch.equal(a.staged, b.staged) and torch.equal(a.staged, b.staged_target)
        assert torch.equal(a.staged_plan, b.staged_plan) and torch.equal(a.staged_offsets, b.staged_offsets)
        assert a.reverb_records_numpy().tobytes() == b.reverb_records_numpy().tobytes()
        s = b.split_records_numpy()
        assert np.array_equal(s["split"], s["ntaps"]) and np.array_equal(s["target_saturated"], s["saturated"])
    assert a.step() == b.step() == 2


def test_a_source_with_a_target_corpus_equals_the_checker():
    import torch
    from gtcrn_micro_amd.data import BatchSource, Corpus
    speech, noise, sp, nz, _ = _corpora()
    rng = np.random.default_rng(4)
    target = [(s // 2 + rng.integers(-50, 50, len(s))).astype(np.int16) for s in speech]
    tg = Corpus.from_arrays(target)
    B, L, seed, item0 = 7, 4099, 11, 14
    src = BatchSource(sp, noise=nz, target=tg, B=B, L=L, seed=seed, item0=item0)
    soff, noff = sp.offsets.cpu().numpy(), nz.offsets.cpu().numpy()
    for step in range(2):
        noisy, clean = src.draw()
        torch.cuda.synchronize()
        plan = src.plan_numpy()
        BC.assert_same_plan(plan, BC.plan(soff, noff, B, L, seed, step, item0=item0))
        wn, wc, wrec = TC.mix_target(np.concatenate(speech), soff, np.concatenate(noise), noff, np.concatenate(target), plan, L)
        assert src.records.cpu().numpy().tobytes() == wrec.tobytes()
        assert np.array_equal(_bits(noisy), wn.view(np.int32)) and np.array_equal(_bits(clean), wc.view(np.int32))


def test_a_captured_draw_with_a_target_replays_consecutive_batches():
    import torch
    from gtcrn_micro_amd.data import BatchSource
    _, _, sp, nz, bank = _corpora()
    B, L = 6, 4099
    kw = dict(noise=nz, B=B, L=L, seed=5, rirs=bank, p_reverb=0.5, target_ms=2.5)
    eager = BatchSource(sp, **kw)
    want = []
    for _ in range(3):
        n, c = eager.draw()
        want.append((n.clone(), c.clone(), eager.plan.clone(), eager.records.clone(), eager.reverb_plan.clone(),
                     eager.split_records.clone(), eager.staged_target.clone()))
    src = BatchSource(sp, **kw)
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
        for got, ref in zip((out[0], out[1], src.plan, src.records, src.reverb_plan, src.split_records, src.staged_target), want[k]):
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), k
    assert src.step() == 3 and eager.step() == 3
    assert not torch.equal(want[0][0], want[1][0]) and not torch.equal(want[0][1], want[0][0])


def test_bad_arguments_are_refused():
    import torch
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd._lib import lib
    from gtcrn_micro_amd.data import BatchSource, Corpus
    speech, noise, sp, nz, bank = _corpora()
    same = Corpus.from_arrays(speech)
    for kw in (dict(noise=nz, target_ms=5.0),                                # target_ms without rirs=
               dict(noise=nz, rirs=bank, p_reverb=0.5, target_ms=-1.0), dict(noise=nz, rirs=bank, p_reverb=0.5, target_ms=float("nan")),
               dict(noise=nz, rirs=bank, p_reverb=0.5, target_ms=float("inf")),
               dict(noise=nz, target=same, rirs=bank, p_reverb=0.5), dict(paired_clean=same, target=same),
               dict(noise=nz, paired_clean=same, target=same), dict(noise=nz, target=nz), dict(noise=nz, target="corpus"),
               dict(noise=nz, target=Corpus.from_arrays([s[:-1] if len(s) > 1 else s for s in speech]))):
        with pytest.raises(GtcrnError):
            BatchSource(sp, B=2, L=100, **kw)
    with pytest.raises(GtcrnError):
        bank.split_table(np.array([1, 2, 3], np.int32))                      # one entry per response
    assert bank.split_table([5, 5, 5, 5])[0] is bank.split_table(np.array([5, 5, 5, 5]))[0]    # kept per split
    K1 = int(np.diff(bank.offsets.cpu().numpy())[1])
    assert bank.split_table([0, 99999, 5, 5])[0].cpu().tolist() == [1, K1, 5, 5]
    # the C entry points on real device buffers: refused before anything is enqueued
    src = BatchSource(sp, noise=nz, B=2, L=100, rirs=bank, p_reverb=0.5, target_ms=5.0)
    args = [sp.pcm.data_ptr(), sp.offsets.data_ptr(), sp.n, bank.taps.data_ptr(), bank.offsets.data_ptr(), src.split.data_ptr(), bank.n,
            src.split_table.data_ptr(), src.split_table.numel(), src.plan.data_ptr(), src.reverb_plan.data_ptr(), 2, 100,
            src.staged.data_ptr(), src.staged_target.data_ptr(), src.staged_stride, src.staged_offsets.data_ptr(),
            src.staged_plan.data_ptr(), src.split_records.data_ptr(), src._rws.data_ptr(), 0, None]
    for pos, val in ((11, 0), (12, 0), (15, 99), (20, 5), (7, None), (13, None), (14, None), (5, None), (6, 0)):
        bad = list(args)
        bad[pos] = val
        assert lib().gtcrn_batch_reverb_split(*bad) == -1, (pos, val)
    assert lib().gtcrn_batch_reverb_split(*args) == 0
    margs = [src.staged.data_ptr(), src.staged_offsets.data_ptr(), 2, nz.pcm.data_ptr(), nz.offsets.data_ptr(), nz.n,
             src.staged_target.data_ptr(), src.staged_plan.data_ptr(), 2, 100, src.noisy.data_ptr(), 100, src.clean.data_ptr(), 100,
             src.records.data_ptr(), src._ws.data_ptr(), 7, None]
    for pos, val in ((6, None), (8, 0), (9, 0), (11, 99), (16, 0), (14, None)):
        bad = list(margs)
        bad[pos] = val
        assert lib().gtcrn_batch_mix_target(*bad) == -1, (pos, val)
    assert lib().gtcrn_batch_mix_target(*margs) == 0
    torch.cuda.synchronize()


def test_new_kernels_use_no_scratch_and_spill_nothing():
    """From the committed resource dump of the kernels this section adds (profiles/reverb_target_resources.txt)."""
    rows = [l for l in open(os.path.join(ROOT, "profiles", "reverb_target_resources.txt")) if not l.startswith("#") and l.strip()]
    names = ["k_split_plain", "k_split_mm<2>", "k_split_mm<8>", "k_split_finish", "k_split_header", "k_split_sum", "k_split_tiles",
             "k_batch_write_target"]
    for n in names:
        assert sum(n in l for l in rows) == 1, n
    assert len(rows) == len(names) and not any("k_reverb_mfma" in l for l in rows)
    for l in rows:
        assert "ScratchSize [bytes/lane]: 0 " in l and "VGPRs Spill: 0 " in l and "SGPRs Spill: 0 " in l, l
