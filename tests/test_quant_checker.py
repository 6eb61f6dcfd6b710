"""The acceptance criterion of the int8-weight / fp16-activation variant (tests/quant_cases.py), on the CPU.

QuantPort(acc="f32") stands in for the kernels and QuantPort(acc="f64") is the reference: the same contract in two
summation orders, whose distance is the flip-noise floor.  The inputs and the acceptance function are the ones
tests/test_gpu_quant_edges.py applies to the kernels.  A third order (float32, every reduction in two halves) stands for
the kernels' independent draw of the same noise: it has to pass at the margin K on every case, and every seeded bug of
oracle/quant_port.py has to fail on at least one."""
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
    assert all(caught.values()), [m for m, v in caught.items() if not v]


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
