"""The acceptance criterion of the int8-weight / fp16-activation variant (tests/quant_cases.py), on the CPU.

QuantPort(acc="f32") stands in for the kernels and QuantPort(acc="f64") is the reference: the same contract in two
summation orders, whose distance is the flip-noise floor.  The inputs and the acceptance function are the ones
tests/test_gpu_quant_edges.py applies to the kernels.  A third order (float32, every reduction in two halves) stands for
the kernels' independent draw of the same noise: it has to pass at the margin K on every case, and every seeded bug of
oracle/quant_port.py has to fail on at least one.

The pinned check (QC.accept_stages) is held the same way: the third order plays the device, stage taps and all; it
has to pass every stage of every stage case, and every seeded bug has to fail in the stage it is seeded in -- on EVERY
stage case where it is active -- and pass every other stage."""
import numpy as np
import pytest

import quant_cases as QC

torch = pytest.importorskip("torch")


def _worst(case, **kw):
    """Evaluate port(**kw) on every seed of `case`: (all accepted, worst ratio to the floor per statistic)."""
    pairs, floors = QC.reference(case)
    ok, worst = True, (0.0, 0.0, 0.0)
    for x, ref, _ in pairs:
        a, _, ratios = QC.accept(QC.port(case.tag, **kw).forward(x, case.in_scale, case.out_scale), ref, floors)
        ok, worst = ok and a, tuple(max(p, q) for p, q in zip(worst, ratios))
    return ok, worst


@pytest.mark.parametrize("tag", ["dns3", "rand"])
def test_unmutated_orders_are_accepted_on_every_case(tag):
    for case in (c for c in QC.CASES if c.tag == tag):
        _, floors = QC.reference(case)
        pairs, _ = QC.reference(case)
        w1 = [QC.accept(f32, ref, floors, k=1.0) for _, ref, f32 in pairs]
        ok3, w3 = _worst(case, split=True)
        print(f"{case.name:24s} floors L2 {floors[0]:.2e} frame {floors[1]:.2e} frac {floors[2]:.2e}; "
              f"third order / floor {w3[0]:.2f} {w3[1]:.2f} {w3[2]:.2f}")
        assert all(a[0] for a in w1), (case, w1)            # by construction, at K = 1
        assert ok3, (case, w3, QC.K)


def test_every_seeded_bug_is_rejected():
    from oracle.quant_port import MUTANTS
    caught = {m: [] for m in MUTANTS}
    for name in QC.MUTANT_CASES:
        case = QC.BY_NAME[name]
        for m in MUTANTS:
            ok, w = _worst(case, mutate=m)
            print(f"{name:24s} {m:18s} / floor {w[0]:8.2f} {w[1]:8.2f} {w[2]:8.2f} {'' if ok else 'rejected'}")
            if not ok:
                caught[m].append(name)
    # the inverse-ERB sum feeds nothing but the mask product: its missed rounding never avalanches, and no output-only
    # criterion sees it on any case (best ratio 3.0, rand-B1-T1); the pinned check holds it (below)
    assert all(v for m, v in caught.items() if m not in QC.PINNED_ONLY_MUTANTS), [m for m, v in caught.items() if not v]


def test_checker_modes():
    """The default is the float32 order; a mutant, the split and the float64 order each change the result; the
    quantiser step is the float32 quotient the library forms, and the host quantiser rounds ties to even and clips at
    -128 / 127."""
    from oracle.quant_port import CALIB_SCALE, int8_boundary, quant_step
    case = QC.BY_NAME["rand-B1-T17-ties"]
    x = case.input(0)
    base = QC.port("rand").forward(x, case.in_scale)
    assert np.array_equal(base, QC.port("rand", "f32", None, False).forward(x, case.in_scale))
    assert not np.array_equal(base, QC.port("rand", mutate="ties_away").forward(x, case.in_scale))
    assert not np.array_equal(base, QC.port("rand", split=True).forward(x, case.in_scale))
    assert not np.array_equal(base, QC.port("rand", "f64").forward(x, case.in_scale))
    assert np.array_equal(base, base.astype(np.float16).astype(np.float32))
    step = quant_step(CALIB_SCALE)
    assert step == np.float32(CALIB_SCALE) / np.float32(255)
    k = np.array([-129.5, -128.5, -127.5, -2.5, -1.5, -0.5, 0.5, 1.5, 2.5, 126.5, 127.5, 300], np.float32)
    q = int8_boundary(torch.from_numpy(k), 255.0).numpy()                    # step 1: every tie is exact
    assert np.array_equal(q, [-128, -128, -128, -2, -2, -0.0, 0, 2, 2, 126, 127, 127])


# ---- the pinned, per-stage check (QC.accept_stages) -----------------------------------------------------------------
def _device(case, seed, **kw):
    """The stand-in device: the two-halves order (with a seeded bug or not), its output and its stage taps."""
    taps = {}
    QC.port(case.tag, split=True, **kw).forward(case.input(seed), case.in_scale, case.out_scale, taps=taps)
    return taps


@pytest.mark.parametrize("tag", ["dns3", "rand"])
def test_pins_and_taps_leave_the_default_alone(tag):
    """Neither argument: the bits of the checker before it had stage code (tests/golden/quant_port_f64_*.f16: its
    float64-order output on the tie case, seed 0, recorded from that version; every value is an fp16 number).  In each
    order: empty pins and a taps dict change nothing; the taps pinned back in reproduce the run; a pin is what
    everything downstream reads, and nothing upstream."""
    import os
    from oracle.quant_port import STAGES
    case = QC.BY_NAME[f"{tag}-B1-T17-ties"]
    x = case.input(0)
    gold = np.fromfile(os.path.join(os.path.dirname(__file__), "golden", f"quant_port_f64_{case.name}.f16"), np.float16)
    assert np.array_equal(QC.port(tag, "f64").forward(x, case.in_scale), gold.astype(np.float32).reshape(1, 257, 17, 2))
    for acc, split in (("f32", False), ("f64", False), ("f32", True)):
        p = QC.port(tag, acc, None, split)
        base, taps = p.forward(x, case.in_scale), {}
        assert np.array_equal(base, p.forward(x, case.in_scale, pins={}, taps=taps)) and tuple(taps) == STAGES
        assert np.array_equal(base, taps["out"])
        assert np.array_equal(base, p.forward(x, case.in_scale, pins=taps))
    assert taps["en0"].shape == (1, 16, 17, 65) and taps["sum4"].shape == (1, 16, 17, 33) and taps["de4"].shape == (1, 2, 17, 129)
    other = {}
    p.forward(x, case.in_scale, pins={"en4": np.zeros_like(taps["en4"])}, taps=other)
    assert np.array_equal(other["en3"], taps["en3"]) and np.array_equal(other["en4"], taps["en4"])
    assert not np.array_equal(other["gtcn1"], taps["gtcn1"]) and not np.array_equal(other["sum4"], taps["sum4"])


@pytest.mark.parametrize("tag", ["dns3", "rand"])
def test_unmutated_device_is_accepted_in_every_stage(tag):
    for case in QC.stage_cases(tag):
        for seed in case.seeds:
            ok, rep = QC.accept_stages(_device(case, seed), case, seed)
            worst = max(rep.items(), key=lambda kv: max(kv[1][2]))
            print(f"{case.name:24s} seed {seed}: worst stage {worst[0]:5s} / floor "
                  f"{worst[1][2][0]:.2f} {worst[1][2][1]:.2f} {worst[1][2][2]:.2f}")
            assert ok, (case, seed, QC.stage_failures(rep))


def _mutants():
    from oracle.quant_port import MUTANTS
    return list(MUTANTS)


@pytest.mark.parametrize("mutant", _mutants())
def test_seeded_bug_is_rejected_in_its_stage_and_in_no_other(mutant):
    """On every stage case where the bug is active (first seed): rejected in the stage it is seeded in, by at least
    twice the margin, and accepted in every other stage -- the check localises.  (The two boundary bugs change the
    quantised spectrogram, which the output stage reads too.)"""
    from oracle.quant_port import BOUNDARY_MUTANTS, MUTANTS
    stage, ran = MUTANTS[mutant][0], 0
    also = ("out",) if mutant in BOUNDARY_MUTANTS else ()
    for tag in ("dns3", "rand"):
        for case in QC.stage_cases(tag):
            if not QC.mutant_active(mutant, case):
                continue
            seed, ran = case.seeds[0], ran + 1
            ok, rep = QC.accept_stages(_device(case, seed, mutate=mutant), case, seed)
            best = max(rep[stage][2])
            print(f"{mutant:20s} {case.name:24s} {stage}: / floor {rep[stage][2][0]:9.1f} {rep[stage][2][1]:9.1f} "
                  f"{rep[stage][2][2]:9.1f}   rejected in {[st for st, r in rep.items() if not r[0]]}")
            assert not rep[stage][0] and best >= 2 * QC.K_STAGE, (mutant, case, stage, rep[stage])
            assert all(r[0] for st, r in rep.items() if st != stage and st not in also), (mutant, case, QC.stage_failures(rep))
    assert ran >= 2, mutant


def test_missed_rounding_passes_at_the_output_and_fails_in_its_stage():
    """The point of the pinned check, on the trained parameters past two chunks: decoder.de_convs.1 without its fp16
    rounding (and its unrounded skip sum) is accepted by the black-box criterion and rejected at de1, nowhere else."""
    case = QC.BY_NAME["dns3-B1-T33"]
    pairs, floors = QC.reference(case)
    for mutant in ("no_round", "skip_unrounded"):
        for seed, (x, ref, _) in zip(case.seeds, pairs):
            got = QC.port("dns3", split=True, mutate=mutant).forward(x)
            assert QC.accept(got, ref, floors)[0], (mutant, seed)
            ok, rep = QC.accept_stages(_device(case, seed, mutate=mutant), case, seed)
            assert [st for st, r in rep.items() if not r[0]] == ["de1"], (mutant, seed, QC.stage_failures(rep))
