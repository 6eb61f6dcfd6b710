"""The fused HybridLoss (gtcrn_train_loss / gtcrn_train_loss_strided: k_hloss_spec, two k_istft, k_sisnr_sums,
k_sisnr_coef, k_sisnr_gwave, the iSTFT adjoint) against a float64 statement of loss.py:30-71, under the rule of
tests/hybrid_loss_checker.py: the inputs a loss goes wrong at (exact zeros, silent utterances, a prediction 40 .. 120 dB
from its target, pred == true), every memory layout, the one-launch limit and the chunked path above it.
Run with -s to print the kernels' ratios to the floors."""
import numpy as np
import pytest

import hybrid_loss_checker as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trainer():
    import gtcrn_micro_amd as G
    return G.Trainer(0)


def _dev(x, frame_major=False):
    """A (B,257,T,2) array on the GPU; frame_major: (B,T,257,2) memory viewed in that shape."""
    import torch
    t = torch.from_numpy(np.array(x)).cuda()            # (a copy: the shared reference inputs are read-only)
    return t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3) if frame_major else t


def _run(trainer, case, seed):
    """(value, gradient, per-utterance terms) of the kernels for one input of `case`, in the case's layout."""
    pred, true = H.reference(case)[0][seed][:2]
    p, t = _dev(pred, case.layout in ("pred", "both")), _dev(true, case.layout in ("true", "both"))
    loss, grad = trainer.hybrid_loss(p, t)
    terms = trainer.hybrid_loss_terms()
    if case.layout in ("pred", "both"):            # the gradient follows pred's memory order: written through strides
        assert grad.stride(2) > grad.stride(1) and grad.stride(3) == 1
    else:
        assert grad.is_contiguous()
    return float(loss), grad.cpu().numpy(), terms


@pytest.mark.parametrize("case", H.CASES, ids=repr)
def test_kernels_are_accepted(trainer, case):
    _, floors = H.reference(case)
    worst, reasons = (0.0,) * 4, []
    for seed in case.seeds:
        value, grad, terms = _run(trainer, case, seed)
        ok, _, ratios, why = H.accept(value, grad, case, seed, terms)
        worst, reasons = tuple(max(a, b) for a, b in zip(worst, ratios)), reasons + why
    print(f"\n{case.name:26s} floors " + " ".join(f"{f:.2e}" for f in floors) + "; kernels / floor "
          + " ".join(f"{r:.2f}" for r in worst) + ("" if H.gradient_defined(case) else "  (gradient: finite only)"))
    assert not reasons, (case, reasons)


def test_value_alone_is_the_same_value(trainer):
    """want_grad=False skips the gradient stores, k_sisnr_gwave and the adjoint; the value's arithmetic is the same."""
    import torch
    for name in ("random-B3-T9", "near_80", "random-B3-T9-fmaj-pred"):
        case = H.BY_NAME[name]
        pred, true = H.reference(case)[0][0][:2]
        p, t = _dev(pred, bool(case.layout)), _dev(true)
        with_grad, g = trainer.hybrid_loss(p, t)
        alone, none = trainer.hybrid_loss(p, t, want_grad=False)
        assert none is None and g is not None and torch.equal(with_grad, alone), name


def test_batch_permutation_permutes_the_gradient_rows(trainer):
    """The spectral gradient is element-wise (its 1/N depends on the batch size only) and the SI-SNR sums are taken per
    utterance in a fixed order: the rows move bit for bit.  The value adds the same numbers in another order."""
    import torch
    case = H.BY_NAME["random-B3-T9"]
    pred, true, L64, _, _ = H.reference(case)[0][0]
    _, g0 = trainer.hybrid_loss(_dev(pred), _dev(true))
    perm = [2, 0, 1]
    l1, g1 = trainer.hybrid_loss(_dev(pred[perm]), _dev(true[perm]))
    assert torch.equal(g1, g0[perm])
    floor = H.reference(case)[1][0]
    assert abs(float(l1) - L64) / max(abs(L64), 1.0) <= H.K_VALUE * floor


@pytest.mark.parametrize("case", H.BIG_CASES, ids=repr)
def test_one_launch_limit_and_chunking(trainer, case):
    """B = 1024: one utterance per thread of k_sisnr_coef's only block, through the trainer.  B = 1025: HybridLoss cuts
    the batch into launches of at most 1024 and weights their means."""
    import torch
    seed = case.seeds[0]
    pred, true = H.reference(case)[0][seed][:2]
    if case.B <= 1024:
        loss, grad = trainer.hybrid_loss(_dev(pred), _dev(true))
    else:
        from gtcrn_micro_amd.loss import HybridLoss
        p = _dev(pred).requires_grad_(True)
        loss = HybridLoss().cuda()(p, _dev(true))
        loss.backward()
        grad = p.grad
    ok, _, ratios, why = H.accept(float(loss.detach()), grad.cpu().numpy(), case, seed)
    print(f"\n{case.name}: kernels / floor " + " ".join(f"{r:.2f}" for r in ratios))
    assert ok, why


def test_no_dependence_on_stale_loss_workspace():
    """The loss workspace (two waveforms, coefficients, partial sums) is reused: after a larger call whose inputs were NaN
    a smaller call on the same trainer is as clean as on a fresh one."""
    import torch
    import gtcrn_micro_amd as G
    tr = G.Trainer(0)
    nan = torch.full((3, 257, 9, 2), float("nan"), device="cuda")
    loss, grad = tr.hybrid_loss(nan, nan.clone())
    assert torch.isnan(loss) and torch.isnan(grad).all()
    case = H.BY_NAME["random-B1-T2"]
    fresh = G.Trainer(0)
    for seed in case.seeds:
        pred, true = H.reference(case)[0][seed][:2]
        l1, g1 = tr.hybrid_loss(_dev(pred), _dev(true))
        ok, _, _, why = H.accept(float(l1), g1.cpu().numpy(), case, seed, tr.hybrid_loss_terms())
        assert ok, why
        l2, g2 = fresh.hybrid_loss(_dev(pred), _dev(true))
        assert torch.equal(l1, l2) and torch.equal(g1, g2)
