"""The acceptance rule of the fused HybridLoss (tests/hybrid_loss_checker.py), on the CPU.

loss_f64 is held against the reference's own train-step fixtures and against finite differences of itself;
loss_kernel_order, the kernels' arithmetic restated in float32, has to be accepted on every case, and each of its seeded
bugs has to be rejected on at least one.  tests/test_gpu_hybrid_loss.py applies the same rule to the kernels.
Run with -s to print floors and ratios."""
import numpy as np
import pytest

import hybrid_loss_checker as H
from conftest import golden

torch = pytest.importorskip("torch")


def _worst(case, bug=None):
    """loss_kernel_order(bug) on every seed of `case`: (all accepted, worst ratio per statistic, reasons)."""
    per_seed, _ = H.reference(case)
    ok, worst, why = True, (0.0,) * 4, []
    for seed, (pred, true, *_) in per_seed.items():
        value, grad, terms = H.loss_kernel_order(pred, true, bug)
        a, _, ratios, w = H.accept(value, grad, case, seed, terms)
        ok, worst, why = ok and a, tuple(max(p, q) for p, q in zip(worst, ratios)), why + w
    return ok, worst, why


@pytest.mark.parametrize("name", ["trainstep_dns3_B3_T12.npz", "trainstep_rand_B3_T12.npz"])
def test_loss_f64_reproduces_the_reference_train_step(name):
    """`loss` and `grad_enh` were written by the reference's own float32 train step: the distance is that step's own
    rounding (1.2e-8 and 1.5e-7 of max|g| measured on dns3), held at ten float32 roundings."""
    g = golden(name)
    value, grad, _ = H.loss_f64(g["enh"], g["clean_spec"])
    ev = abs(value - float(g["loss"])) / abs(value)
    eg = float(np.abs(grad - g["grad_enh"]).max() / np.abs(grad).max())
    print(f"{name}: value {ev:.2e}, gradient {eg:.2e} of max|g|")
    assert ev < 6e-7 and eg < 6e-7, (ev, eg)


@pytest.mark.parametrize("name", ["random-B3-T9", "zero_bins"])
def test_loss_f64_gradient_is_its_own_finite_difference(name):
    """Central differences (five-point stencil) of loss_f64's value, in float64, on 20 random elements.  Elements that
    are exactly zero sit where the 1e-12 rounds off the magnitude's kink over a width of 1e-6: the step there is 3e-8,
    elsewhere 1e-3 of the element.  Bound: the truncation is ~(h / width)^4 <= 1e-6, the rounding of four values near 10
    in double over 12 h is <= 1e-7 absolute, against a denominator of at least 1e-3 of the utterance's largest gradient
    element."""
    case = H.BY_NAME[name]
    pred, true, _, g64, _ = H.reference(case)[0][case.seeds[0]]
    rng = np.random.default_rng(7)
    worst = 0.0
    for flat in rng.choice(pred.size, 20, replace=False):
        idx = np.unravel_index(flat, pred.shape)
        h = 3e-8 if pred[idx[:3]].tolist() == [0.0, 0.0] else 1e-3 * max(abs(float(pred[idx])), 1e-2)
        f = {}
        for k in (-2, -1, 1, 2):
            p = pred.astype(np.float64)
            p[idx] += k * h
            f[k] = H.loss_f64(p, true)[0]
        fd = (-f[2] + 8 * f[1] - 8 * f[-1] + f[-2]) / (12 * h)
        worst = max(worst, abs(fd - g64[idx]) / max(abs(g64[idx]), 1e-3 * np.abs(g64[idx[0]]).max()))
    print(f"{name}: worst finite-difference mismatch {worst:.2e}")
    assert worst < 1e-5, worst


def test_floor_meets_the_absolute_conditions():
    """loss_f32 (the floor's numerator) is finite on every case and exact where the rule asks for exactness."""
    for case in H.CASES:
        for seed, (pred, true, L64, g64, t64) in H.reference(case)[0].items():
            value, grad = H.loss_f32(pred, true)
            assert np.isfinite(value) and np.isfinite(grad).all() and np.isfinite(L64) and np.isfinite(g64).all(), case
            if case.kind == "both_silent":
                assert abs(value - 8.0) <= 1e-6 and abs(L64 - 8.0) <= 1e-6 and not grad.any() and not g64.any()
            if case.kind in ("silent_target", "silent_pred"):
                assert abs(t64[1 if case.kind == "silent_target" else 2] - 8.0) <= 1e-6


def test_kernel_order_is_accepted_on_every_case():
    for case in H.CASES:
        _, floors = H.reference(case)
        ok, w, why = _worst(case)
        print(f"{case.name:24s} floors " + " ".join(f"{f:.2e}" for f in floors) + "; kernel order / floor "
              + " ".join(f"{r:.2f}" for r in w) + ("" if H.gradient_defined(case) else "  (gradient: finite only)"))
        assert ok, (case, why)
    # the cases where only the value is held are the ones the rule names, not more
    assert {c.name for c in H.CASES if not H.gradient_defined(c)} <= {"near_100", "near_120", "identical"}


def test_every_seeded_bug_is_rejected():
    cases = [c for c in H.CASES if not c.layout]
    caught = {b: [] for b in H.BUGS}
    for bug in H.BUGS:
        for case in cases:
            ok, w, _ = _worst(case, bug)
            print(f"{bug:15s} {case.name:16s} / floor " + " ".join(f"{r:9.3g}" for r in w) + ("" if ok else "  rejected"))
            if not ok:
                caught[bug].append(case.name)
    assert all(caught.values()), [b for b, v in caught.items() if not v]
    # the arithmetic the kernels had: the residual from float32-rounded products
    assert {"near_80", "near_100", "near_120"} <= set(caught["f32_products"]), caught["f32_products"]
    # the two epsilons carry exactly the inputs they were put there for
    assert "zero_bins" in caught["no_eps_mag"] and "silent_target" in caught["no_eps_proj"]
