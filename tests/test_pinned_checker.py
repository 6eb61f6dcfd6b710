"""The pinned float64 checker of the bf16 train step (oracle/pinned_check.py), on the CPU.

The float32 run of the port's bf16-storage graph stands in for the device: it stores the same tensors, rounded the
same way, in another arithmetic.  Against the float64 run of the same graph it shows why the checker has to be pinned
(unpinned, rounding flips compound along the 46-unit chain to ~0.2 relative in gradient) and how tight it is once
pinned to the stand-in's stored tensors (every unit then sees the inputs the stand-in's unit saw).  The bounds are
about 4x what was measured here (ATen's summation order differs between machines and thread counts); each seeded
unit bug must fail the same check the GPU test applies to the trainer's gradient."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden")

# measured (B = 3 x T = 12 | B = 8 x T = 251): blob 3.7e-6 | 9.1e-6; worst tensor of >= 16 elements 2.3e-5 | 5.4e-5;
# worst of fewer (PReLU slopes, 8-/2-channel biases) 7.3e-5 | 7.9e-5; near-zero truths (conv biases in front of a
# train-mode BatchNorm) 8.5e-7 | 2.6e-6 of max|g|
BOUNDS = {(3, 12): (2e-5, 1e-4, 3e-4, 4e-6), (8, 251): (4e-5, 2.5e-4, 3e-4, 1e-5)}


def _case(B, T):
    import torch
    torch.set_num_threads(min(8, torch.get_num_threads()))
    blob = np.fromfile(os.path.join(GOLD, "params_dns3.f32"), np.float32)
    rng = np.random.default_rng(12)
    spec = (rng.standard_normal((B, 257, T, 2)) * 0.3).astype(np.float32)
    gout = (rng.standard_normal((B, 257, T, 2)) * 0.01).astype(np.float32)
    return blob, spec, gout


@pytest.mark.parametrize("B,T", [(3, 12), (8, 251)])
def test_pinned_checker_holds_the_float32_stand_in_per_unit(B, T):
    from oracle import pinned_check as PC
    blob, spec, gout = _case(B, T)
    taps, _, g32, _ = PC.record(blob, spec, gout)
    # unpinned: the two evaluations of the same bf16 network part at the first rounding flip
    _, _, g64u, _ = PC.pinned_truth(blob, spec, gout, None)
    e_unpinned = float(np.linalg.norm(g32 - g64u) / np.linalg.norm(g64u))
    mine, _, g64, _ = PC.pinned_truth(blob, spec, gout, taps)
    e_all, rows, fails = PC.check_grads(g32, g64, *BOUNDS[(B, T)])
    print(f"B={B} T={T}: unpinned blob rel-L2 {e_unpinned:.3f}; pinned: {PC.summary(e_all, rows)}")
    assert e_unpinned > 0.1
    assert not fails, fails
    # every stored tensor (71: each unit's centred conv output, block outputs, decoder sums) is pinned, and the
    # checker's own value of it is the stored one or the adjacent bf16 value; a few elements further off are
    # downstream of an activation that rounded the other way (lean units do not store theirs: it is not pinned)
    assert len(taps) == 71 and all(n + ".y" in taps for n in {r[0].rsplit(".", 1)[0] for r in rows if "bn" in r[0]})
    n_all = sum(v.numel() for v in taps.values())
    agree = PC.forward_agreement(mine, taps)
    far = sum(v[1] for v in agree.values()) / n_all
    worst = max(agree.items(), key=lambda kv: kv[1][0])
    print(f"forward: worst adjacent share {worst[0]} {worst[1][0]:.2e}; elements further apart {far:.1e}")
    assert worst[1][0] < 3e-3 and far < 1e-4


def test_pinned_checker_rejects_seeded_unit_bugs():
    """BN weight gradient x1.01, one PReLU slope's x1.05, one depthwise tap zeroed: each fails the pinned check (and
    the unmutated gradient passes it), at B = 3 x T = 12."""
    from oracle import pinned_check as PC
    blob, spec, gout = _case(3, 12)
    taps, _, g32, _ = PC.record(blob, spec, gout)
    _, _, g64, _ = PC.pinned_truth(blob, spec, gout, taps)
    assert not PC.check_grads(g32, g64, *BOUNDS[(3, 12)])[2]
    for name, g in PC.mutations(g32, g64):
        fails = PC.check_grads(g, g64, *BOUNDS[(3, 12)])[2]
        assert name in [f[0] for f in fails], (name, fails)


def test_bf16_gradient_hand_offs_in_the_checker():
    """grad_round=True rounds the gradient to bf16 at the hand-offs the trainer stores in bf16 (storage "bf16_grads").
    Those roundings cannot be pinned, so what is left is their noise: blob ~6e-3 (measured 6.0e-3 here), well under the
    unpinned 0.2; the forward is the bf16 mode's (same taps)."""
    from oracle import pinned_check as PC
    blob, spec, gout = _case(3, 12)
    taps, _, g32, _ = PC.record(blob, spec, gout, grad_round=True)
    taps_plain, _, g32_plain, _ = PC.record(blob, spec, gout)
    assert all(np.array_equal(taps[n].numpy(), taps_plain[n].numpy()) for n in taps)
    _, _, g64, _ = PC.pinned_truth(blob, spec, gout, taps, grad_round=True)
    e_all = float(np.linalg.norm(g32 - g64) / np.linalg.norm(g64))
    e_plain = float(np.linalg.norm(g32_plain - g64) / np.linalg.norm(g64))
    print(f"bf16 gradient hand-offs: pinned blob rel-L2 {e_all:.2e} (plain bf16 stand-in against it {e_plain:.2e})")
    assert 1e-3 < e_all < 1.5e-2 and e_plain > 1e-3      # the rounding is modelled, and it is there
