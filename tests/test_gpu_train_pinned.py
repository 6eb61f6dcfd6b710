"""The bf16 train step (BASELINE configs[3], the step bench.py times) unit by unit against the float64 checker PINNED to
what the trainer stored (oracle/pinned_check.py).

After tr.forward every stored tensor is read through the trainer's taps (each unit's centred bf16 conv output
"<bn prefix>.y", the block outputs, the decoder sums).  The float64 port of the bf16-storage graph then runs with each of
them snapped in at the point where the trainer wrote it, v + (stored - v).detach(): every unit of the checker sees
exactly the inputs the HIP unit saw, and rounding flips no longer compound along the chain.  Held per unit:
  * forward: the checker's own value of every stored tensor is the trainer's or the adjacent bf16 value (a small share;
    a few elements further off sit behind an activation that rounded the other way -- lean units do not store theirs);
  * gradient: blob rel-L2, rel-L2 of every trainable tensor with a nonzero truth whatever its size, and for the conv
    biases in front of a train-mode BatchNorm (true gradient ~0) an absolute bound scaled to max|g|;
  * running statistics after the step;
  * the same check rejects seeded unit bugs applied to the trainer's gradient.
Storage "bf16_grads" rounds the gradients handed between units as well; the checker rounds them at the same hand-offs
(grad_round=True), but those roundings cannot be pinned, so its bounds are the level of that noise (the CPU stand-in
measures the same, tests/test_pinned_checker.py).  Fusion masks: all (65535), the layer-at-a-time passes (0; 16 -- skip
gradients accumulated in place -- for "bf16_grads", which needs that bit), and all but normalise-on-load and the
recomputed activations (bits 1 and 8).

The fp32 storage mode (the default, what GTCRNMicro.train() runs and "bf16_saves" is held to) is checked the same way:
every "<bn prefix>.y" is then the plain fp32 conv output, and the pinned float64 checker sees the inputs each HIP unit
saw, so a PReLU element on the other side of its kink no longer parts the two gradients (unpinned: up to 1e-2 in blob
rel-L2 at some inputs, tests/test_pinned_checker.py).  Its cases sit round the tilings -- the 8- and 12-frame tiles with
two-frame halos, the 32-frame tile of train_kernels.hip, the TCN's dilations -- under four fusion masks, with finer
seeded bugs, one of them the upstream gradient of a single frame lost (a dropped halo frame)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")

MASKS = {"all": 65535, "none": 0, "no_load_norm": 65535 & ~(1 | 8)}


def _inputs(shape):
    if shape == "big":
        blob_np = np.fromfile(os.path.join(GOLD, "params_dns3.f32"), np.float32)
        rng = np.random.default_rng(12)
        spec = (rng.standard_normal((8, 257, 251, 2)) * 0.3).astype(np.float32)
        gout = (rng.standard_normal((8, 257, 251, 2)) * 0.01).astype(np.float32)
        return blob_np, spec, gout
    g = np.load(os.path.join(GOLD, f"trainstep_{shape}_B3_T12.npz"))
    return np.fromfile(os.path.join(GOLD, f"params_{shape}.f32"), np.float32), g["noisy_spec"], g["grad_enh"]


@pytest.mark.parametrize("shape", ["dns3", "rand", "big"])
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("storage", ["bf16", "bf16_grads"])
def test_bf16_train_step_per_unit_against_the_pinned_checker(storage, mask, shape):
    import torch
    from gtcrn_micro_amd import Trainer
    from oracle import pinned_check as PC
    torch.set_num_threads(min(8, torch.get_num_threads()))
    blob_np, spec_np, gout_np = _inputs(shape)
    fusions = MASKS[mask] if (storage != "bf16_grads" or MASKS[mask] & 16) else 16
    tr = Trainer(0)                     # fresh: the centring shifts are the running means, as in the checker
    tr.set_storage(storage)
    tr.set_fusions(fusions)
    blob = torch.from_numpy(blob_np.copy()).cuda()
    spec = torch.from_numpy(spec_np).cuda()
    out = tr.forward(blob, spec)
    taps = PC.read_taps(tr, fusions)
    grads = tr.backward(blob, spec, torch.from_numpy(gout_np).cuda())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grads).all())
    PC.assert_pinned_step(storage, blob_np, spec_np, gout_np, taps, grads.cpu().numpy(),
                          blob.cpu().numpy().astype(np.float64), out.cpu().numpy(), f"{storage} fusions {fusions} {shape}")
    tr.close()


# 65535: the default; 0: layer-at-a-time; no normalise-on-load, no recomputed activations; 1023: the LDS-tiled backward
# passes without the in-launch finishes, sums in the producer, k_pw_fwd, the column depthwise and the batched finishes
F32_MASKS = {"all": 65535, "none": 0, "no_load_norm": 65535 & ~(1 | 8), "round4": 1023}


def _f32_shapes():
    from oracle import pinned_check as PC
    return PC.F32_SHAPES


@pytest.mark.parametrize("B,T", _f32_shapes())
@pytest.mark.parametrize("mask", list(F32_MASKS))
@pytest.mark.parametrize("tag", ["dns3", "rand"])
def test_f32_train_step_per_unit_against_the_pinned_checker(tag, mask, B, T):
    import torch
    from gtcrn_micro_amd import Trainer
    from oracle import pinned_check as PC
    torch.set_num_threads(min(8, torch.get_num_threads()))
    blob_np, spec_np, gout_np = PC.f32_inputs(tag, B, T)
    fusions = F32_MASKS[mask]
    tr = Trainer(0)
    tr.set_storage("f32")
    tr.set_fusions(fusions)
    blob = torch.from_numpy(blob_np.copy()).cuda()
    spec = torch.from_numpy(spec_np).cuda()
    out = tr.forward(blob, spec)
    taps = PC.read_taps(tr, fusions)
    grads = tr.backward(blob, spec, torch.from_numpy(gout_np).cuda())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grads).all())
    assert len(taps) == (65 if fusions & 2048 else 71)      # (bit 11: the six sum-minus-skip taps give way to the sums)
    PC.assert_pinned_step("f32", blob_np, spec_np, gout_np, taps, grads.cpu().numpy(),
                          blob.cpu().numpy().astype(np.float64), out.cpu().numpy(), f"f32 fusions {fusions} {tag} {B}x{T}",
                          lost_frame=PC.F32_LOST_FRAME.get((B, T)))
    tr.close()


def test_unit_taps_are_the_stored_tensors():
    """The taps the pinned check reads: every unit's y in the shape of its conv output, tcn3 / tcn7 equal gtcn1 / gtcn2,
    all of them bf16 values, and a stored sum is what the next layer read (sum4 = de3 + en0 rounded, bit for bit; with
    fusion bit 11 off the bf16 modes keep only the last sum)."""
    import torch
    from gtcrn_micro_amd import Trainer
    from oracle import pinned_check as PC
    blob_np, spec_np, _ = _inputs("dns3")
    tr = Trainer(0)
    tr.set_storage("bf16")
    tr.set_fusions(2047)
    blob = torch.from_numpy(blob_np.copy()).cuda()
    tr.forward(blob, torch.from_numpy(spec_np).cuda())
    taps = PC.read_taps(tr, 2047)
    assert len(taps) == 67                           # 46 y + 5 + 8 + 2 + the last sum + 5 (shared sum buffer)
    assert taps["gtcn2.blocks.2.bn2.y"].shape == (3, 16, 12, 33)
    assert taps["decoder.de_convs.1.point_bn2.y"].shape == (3, 8, 14, 33)
    assert taps["decoder.de_convs.4.bn.y"].shape == (3, 2, 12, 129)
    assert torch.equal(taps["tcn3"], taps["gtcn1"]) and torch.equal(taps["tcn7"], taps["gtcn2"])
    s4 = (taps["de3"] + taps["en0"]).float().to(torch.bfloat16).double()
    assert torch.equal(taps["sum4"], s4)
    for v in taps.values():                          # bf16 values, handed out as floats
        assert torch.equal(v, v.float().to(torch.bfloat16).double())
    tr.close()
