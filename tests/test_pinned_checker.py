"""The pinned float64 checker of the bf16 train step (oracle/pinned_check.py), on the CPU.

The float32 run of the port's bf16-storage graph stands in for the device: it stores the same tensors, rounded the
same way, in another arithmetic.  Against the float64 run of the same graph it shows why the checker has to be pinned
(unpinned, rounding flips compound along the 46-unit chain to ~0.2 relative in gradient) and how tight it is once
pinned to the stand-in's stored tensors (every unit then sees the inputs the stand-in's unit saw).  The bounds are
about 4x what was measured here (ATen's summation order differs between machines and thread counts); each seeded
unit bug must fail the same check the GPU test applies to the trainer's gradient.

The fp32 storage mode the same way: the float32 run of the port's plain graph (store=None) stands in for the device at
every case of the GPU test.  No stored tensor is rounded there, yet at some inputs an element lands on the other side of
a kink in one of the two arithmetics and the unpinned gradients part by more than 1e-3; pinned they agree to ~1e-6."""
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


# ---- fp32 storage: the float32 port (store=None) as the stand-in, at the cases of the GPU test ----------------------
# measured here (8 threads), worst over dns3 / rand and every shape; the bounds are ~4x:
#   blob 2.4e-6 (dns3 2 x 251); tensor of >= 16 elements 6.9e-5 en_convs.3.point_bn1.weight (rand 2 x 251); of fewer
#   8.0e-4 en_convs.2.point_act.weight (rand 1 x 33); the 46 conv biases in front of a BatchNorm 4.2e-6 of max|g|
#   (en_convs.0.conv.bias, rand 2 x 251); the TCN's depthwise weights with dilation >= T (PC.f32_cancelling) 2.1e-3
#   gtcn2.blocks.2.conv2.weight (dns3 2 x 3; 1.3e-3 gtcn1.blocks.3.conv2.weight at 2 x 7 and 1 x 8)
#   forward, checker's own value against the stored tensor: 6.9e-7 de_convs.1.depth_bn.y; output 1.04e-7; running
#   statistics 1.4e-7
#   unpinned blob rel-L2: rand 1 x 8 1.3e-2, rand 1 x 40 3.0e-3, rand 2 x 251 2.2e-3 (dns3 1 x 40 9.3e-4, 2 x 251 8.1e-4;
#   every other case 1e-6 .. 2e-5); lost frame: 0.11 / 0.088 of the gradient at 2 x 37, 0.035 / 0.018 at 2 x 251
F32_BOUNDS, F32_CANCELLING = (1e-5, 2.8e-4, 3.2e-3, 1.7e-5, None), 8.4e-3
F32_FWD, F32_OUT, F32_STATS = 2.8e-6, 4.2e-7, 5.6e-7
F32_PARTS_UNPINNED = {("rand", 1, 8), ("rand", 2, 251)}


def _f32_cases():
    from oracle import pinned_check as PC
    return [(tag, B, T) for tag in ("dns3", "rand") for B, T in PC.F32_SHAPES]


@pytest.mark.parametrize("tag,B,T", _f32_cases())
def test_pinned_checker_holds_the_float32_stand_in_of_the_f32_step(tag, B, T):
    """Pinned to the stand-in's 71 stored fp32 tensors, the float64 checker accepts its gradient tensor by tensor and
    rejects every seeded bug -- BatchNorm weight x1.002, a PReLU slope x1.005, a depthwise tap zeroed, the upstream
    gradient of one frame lost; unpinned, two of the cases part by more than 1e-3."""
    import torch
    from oracle import pinned_check as PC
    torch.set_num_threads(min(8, torch.get_num_threads()))
    blob, spec, gout = PC.f32_inputs(tag, B, T)
    taps, enh32, g32, blob32 = PC.record(blob, spec, gout, storage="f32")
    assert len(taps) == 71 and sorted(taps) == sorted(PC.tap_names())        # every point the trainer stores is reached
    if (tag, B, T) in F32_PARTS_UNPINNED:
        g64u = PC.pinned_truth(blob, spec, gout, None, storage="f32")[2]
        e_unpinned = float(np.linalg.norm(g32 - g64u) / np.linalg.norm(g64u))
        print(f"{tag} B={B} T={T}: unpinned blob rel-L2 {e_unpinned:.2e}")
        assert e_unpinned > 1e-3
    lost_frame = PC.F32_LOST_FRAME.get((B, T))
    fig = PC.f32_figures(blob, spec, gout, taps, g32, blob32.astype(np.float64), enh32, F32_BOUNDS, F32_CANCELLING,
                         lost_frame, f"{tag} B={B} T={T}")
    assert not fig["fails"], fig["fails"]
    assert fig["fwd"][1] < F32_FWD and fig["out"] < F32_OUT and fig["stats"] < F32_STATS
    assert len(fig["caught"]) == (3 if lost_frame is None else 4) and all(fig["caught"].values()), fig["caught"]
    assert lost_frame is None or fig["lost_share"] > 1e-2


def test_f32_check_holds_every_live_tensor_by_its_rel_l2():
    """Only the 46 conv biases in front of a BatchNorm are held by the absolute bound in the fp32 check, however small
    another tensor's truth is: a tensor at 1e-5 of max|g| that is wrong by 1 % fails, where the bf16 check's
    near-zero class (below 1e-4 of max|g|) lets it pass."""
    from oracle import pinned_check as PC
    from oracle.torch_port import is_trainable
    tab = {n: (k, o) for n, k, o in PC.param_table()}
    biases = PC.conv_biases_before_bn()
    assert len(biases) == 46 and biases <= set(tab)
    rng = np.random.default_rng(0)
    truth = rng.standard_normal(sum(k for k, _ in tab.values()))
    for n in biases:
        truth[tab[n][1]:tab[n][1] + tab[n][0]] = 0.0
    k, o = tab["gtcn1.blocks.3.conv2.weight"]
    truth[o:o + k] *= 1e-5
    got = truth.copy()
    got[o:o + k] *= 1.01
    how = dict(abs_class=biases, special={n: PC.F32_CANCELLING for n in PC.f32_cancelling(7)})
    assert "gtcn1.blocks.3.conv2.weight" in how["special"] and "gtcn1.blocks.2.conv2.weight" not in how["special"]
    _, rows, fails = PC.check_grads(got, truth, *PC.BOUNDS["f32"], **how)
    assert [f[0] for f in fails] == ["gtcn1.blocks.3.conv2.weight"]
    assert {r[0] for r in rows if r[4]} == biases and len(rows) == sum(is_trainable(n) for n in tab)
    assert not PC.check_grads(got, truth, *PC.BOUNDS["f32"])[2]              # (the threshold class: passes)
