"""Unit-level checker of the train step (bf16 and fp32 storage): the float64 port pinned to the tensors the trainer stored.

TEST INFRASTRUCTURE ONLY, like everything under oracle/.
Without pins, one bf16 rounding flip early in the 46-unit chain moves the whole downstream forward, and even the same
bf16 network evaluated in fp32 and in float64 ends 0.2 .. 0.4 apart in gradient.  Pinned (TorchPort(pin=...)), every
unit of the float64 checker sees exactly the inputs the trainer's unit saw, so what is left between the two gradients is
the arithmetic of the units themselves -- small enough to catch a unit that is wrong by a few per cent.
The fp32 storage mode (storage "f32": the port with store=None, every "<bn prefix>.y" the plain conv output) has no
rounding of a stored tensor to flip, but an element of the float32 run that lands on the other side of a kink (PReLU at
0) still parts the two gradients by 1e-3 .. 1e-2 at some inputs; pinned the same way the two agree to ~1e-6, and a unit
that is wrong by 0.2 % is caught.
"""
import os

import numpy as np
import torch

from oracle.torch_port import TorchPort

# fusion bit 11 (not in storage mode 4): these outputs are stored only as a sum with a skip, and their tap is
# sum - skip -- not what any kernel read: the sums sum0 .. sum4 are pinned instead
SUM_MINUS_TAPS = ("gtcn2", "tcn7", "de0", "de1", "de2", "de3")


def param_table():
    import json
    from oracle.torch_port import _MANIFEST
    return [(n, int(np.prod(s)), int(o)) for n, s, o in json.load(open(_MANIFEST))["tensors"]]


# the port's `store` for the trainer's storage mode ("f32": nothing is rounded where it is stored)
PORT_STORE = {"f32": None, "bf16": "bf16", "bf16_grads": "bf16"}


def record(blob, spec, grad_enh, dtype=torch.float32, grad_round=False, storage="bf16"):
    """The float32 stand-in for the device: its forward taps (every stored tensor by name) and its gradient."""
    taps = {}
    port = TorchPort(np.asarray(blob, np.float32).copy(), train=True, dtype=dtype, store=PORT_STORE[storage],
                     grad_round=grad_round)
    enh, grads = port.backward_from(spec, grad_enh, taps=taps)
    return taps, enh, grads, port.blob()


def pinned_truth(blob, spec, grad_enh, pins, grad_round=False, storage="bf16"):
    """The float64 checker pinned to `pins`: (its own pre-snap values of every stored tensor, forward output, gradient
    blob, blob after the step -- running statistics updated)."""
    taps = {}
    port = TorchPort(np.asarray(blob, np.float32).copy(), train=True, dtype=torch.float64, store=PORT_STORE[storage],
                     pin=pins, grad_round=grad_round)
    enh, grads = port.backward_from(spec, grad_enh, taps=taps)
    return taps, enh, grads.astype(np.float64), _blob64(port)


def lost_frame_gradient(blob, spec, grad_enh, pins, t, storage="f32"):
    """The float64 gradient of the upstream gradient restricted to frame `t` of clip 0 (the backward is linear in it):
    what a gradient that lost that frame -- a dropped halo frame -- is short of."""
    one = np.zeros_like(np.asarray(grad_enh))
    one[0, :, t] = np.asarray(grad_enh)[0, :, t]
    return pinned_truth(blob, spec, one, pins, storage=storage)[2]


def _blob64(port):
    return np.concatenate([port.p[n].detach().double().numpy().ravel() for n, _, _ in param_table()])


def bf16_ulps(a, b):
    """Distance in bf16 steps between two arrays of bf16-representable values (as float32 / float64)."""
    def ordered(x):
        i = (np.asarray(x, np.float32).view(np.int32) >> 16).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFF), i)
    return np.abs(ordered(a) - ordered(b))


def forward_agreement(mine, theirs):
    """Per stored tensor: (share of elements one bf16 step apart, count of elements further apart).  `mine`: the
    checker's pre-snap values, `theirs`: the stored values it was pinned to."""
    out = {}
    for name, t in theirs.items():
        d = bf16_ulps(np.asarray(mine[name]), np.asarray(t))
        out[name] = (float((d == 1).mean()), int((d > 1).sum()))
    return out


def forward_rel(mine, theirs):
    """Per stored tensor of the fp32 mode: max|checker's pre-snap value - stored| / max|stored|."""
    out = {}
    for name, t in theirs.items():
        t = np.asarray(t, np.float64)
        out[name] = float(np.abs(np.asarray(mine[name], np.float64) - t).max() / np.abs(t).max())
    return out


def grad_report(got, truth, abs_class=None):
    """Per trainable tensor with a gradient: (name, numel, rel-L2, max|err| / max|truth of the blob|, near-zero truth).
    abs_class (a set of names): the near-zero truths are these tensors and those whose truth is exactly 0, nothing
    else -- not whatever happens to be small."""
    from oracle.torch_port import is_trainable
    got = np.asarray(got, np.float64)
    truth = np.asarray(truth, np.float64)
    gmax = float(np.abs(truth).max())
    rows = []
    for name, numel, off in param_table():
        if not is_trainable(name):
            continue
        t, a = truth[off:off + numel], got[off:off + numel]
        tn = float(np.linalg.norm(t))
        rel = float(np.linalg.norm(a - t) / tn) if tn > 0 else float("inf")
        ab = float(np.abs(a - t).max() / gmax)
        # conv biases in front of a train-mode BatchNorm: true gradient ~0 (rounding noise of the centring), rel-L2 meaningless
        near0 = float(np.abs(t).max()) < 1e-4 * gmax if abs_class is None else (name in abs_class or tn == 0)
        rows.append((name, numel, rel, ab, near0))
    return rows


def check_grads(got, truth, blob_bound, tensor_bound, small_bound, abs_bound, small_abs=None, abs_class=None,
                special=None):
    """The pinned gradient check: blob rel-L2 <= blob_bound; per tensor rel-L2 <= tensor_bound (>= 16 elements) or
    small_bound (fewer: biases of the 2-/8-channel layers, PReLU slopes); tensors whose truth is ~0 instead
    max|err| <= abs_bound * max|truth|.  small_abs (instead of small_bound): the tensors of fewer than 16 elements are
    held by max|err| <= small_abs * max|truth| -- for the noise of unpinnable gradient roundings, which a scalar's
    rel-L2 does not average.  abs_class: see grad_report; special: {name: rel-L2 bound of its own}.
    Returns (blob rel-L2, report rows, failures)."""
    got = np.asarray(got, np.float64)
    truth = np.asarray(truth, np.float64)
    e_all = float(np.linalg.norm(got - truth) / np.linalg.norm(truth))
    rows = grad_report(got, truth, abs_class)
    special = special or {}
    fails = []
    if not e_all <= blob_bound:
        fails.append(("<blob>", e_all, blob_bound))
    for name, numel, rel, ab, near0 in rows:
        if near0:
            if not ab <= abs_bound:
                fails.append((name, ab, abs_bound))
        elif name in special:
            if not rel <= special[name]:
                fails.append((name, rel, special[name]))
        elif numel < 16 and small_abs is not None:
            if not ab <= small_abs:
                fails.append((name, ab, small_abs))
        elif not rel <= (tensor_bound if numel >= 16 else small_bound):
            fails.append((name, rel, tensor_bound if numel >= 16 else small_bound))
    return e_all, rows, fails


def summary(e_all, rows):
    big = [r for r in rows if not r[4] and r[1] >= 16]
    small = [r for r in rows if not r[4] and r[1] < 16]
    near0 = [r for r in rows if r[4]]
    w_big = max(big, key=lambda r: r[2])
    w_small = max(small, key=lambda r: r[2])
    w_0 = max(near0, key=lambda r: r[3]) if near0 else ("-", 0, 0.0, 0.0, True)
    return (f"blob rel-L2 {e_all:.2e}; median per tensor {np.median([r[2] for r in big + small]):.2e}; worst >= 16 el. "
            f"{w_big[0]} {w_big[2]:.2e}; worst < 16 el. {w_small[0]} {w_small[2]:.2e}; worst near-zero truth "
            f"{w_0[0]} {w_0[3]:.1e} of max|g| ({len(near0)} tensors)")


LOST_FRAME = "<lost frame>"


def mutations(got, truth, f_bn=1.01, f_slope=1.05, tap=0, lost=None):
    """Seeded unit bugs, applied to a gradient blob: one BatchNorm weight vector x1.01, one PReLU slope x1.05 (the one
    with the largest true gradient), one depthwise-weight tap (all channels) zeroed; with `lost` (lost_frame_gradient)
    the upstream gradient of one frame lost as well."""
    tab = {n: (k, o) for n, k, o in param_table()}
    truth = np.asarray(truth, np.float64)
    out = []
    g = np.array(got, np.float64, copy=True)
    k, o = tab["gtcn1.blocks.2.bn2.weight"]
    g[o:o + k] *= f_bn
    out.append(("gtcn1.blocks.2.bn2.weight", g))
    slopes = [n for n, (k, _) in tab.items() if k == 1 and "act" in n.split(".")[-2]]
    slope = max(slopes, key=lambda n: abs(truth[tab[n][1]]))
    g = np.array(got, np.float64, copy=True)
    g[tab[slope][1]] *= f_slope
    out.append((slope, g))
    g = np.array(got, np.float64, copy=True)
    k, o = tab["gtcn2.blocks.1.conv2.weight"]          # (16, 1, 3, 1): one tap of every channel
    g[o:o + k].reshape(16, 3)[:, tap] = 0.0
    out.append(("gtcn2.blocks.1.conv2.weight", g))
    if lost is not None:
        out.append((LOST_FRAME, np.asarray(got, np.float64) - np.asarray(lost, np.float64)))
    return out


def mutations_f32(got, truth, lost=None):
    """The finer seeded bugs of the fp32 mode: x1.002 and x1.005, the zeroed tap the one of the current frame -- the
    only one that sees no padding at T = 1."""
    return mutations(got, truth, 1.002, 1.005, 2, lost)


def rejected(name, fails):
    """Whether the failures of a check hold the seeded bug `name`.  The lost frame touches every tensor and counts as
    rejected on any failure: at 2 - 10 % of the gradient it is the blob bound that catches it, which says nothing about
    a single tensor -- the three unit bugs do that."""
    return bool(fails) if name == LOST_FRAME else name in [f[0] for f in fails]


# The cases of the fp32 check (tests/test_gpu_train_pinned.py, and its float32 stand-in in tests/test_pinned_checker.py):
# round the 8- and 12-frame tiles with two-frame halos of the train kernels, the 32-frame tile of train_kernels.hip and
# the TCN's dilations 1, 2, 4, 8 (receptive field 2 x 15 frames per stack)
F32_SHAPES = [(1, 1), (1, 2), (2, 3), (2, 7), (1, 8), (1, 9), (3, 12), (1, 13), (3, 23), (2, 24), (1, 25), (2, 31),
              (1, 32), (1, 33), (2, 37), (5, 13), (1, 40), (2, 65), (2, 251)]
F32_LOST_FRAME = {(2, 37): 8, (2, 251): 12}            # (B, T): the frame of clip 0 whose upstream gradient is lost
_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")


def f32_inputs(tag, B, T):
    """(parameter blob, noisy spectrogram, upstream gradient) of one case: the goldens at B = 3 x T = 12, seeded
    otherwise."""
    blob = np.fromfile(os.path.join(_GOLD, f"params_{tag}.f32"), np.float32)
    if (B, T) == (3, 12):
        g = np.load(os.path.join(_GOLD, f"trainstep_{tag}_B3_T12.npz"))
        return blob, g["noisy_spec"], g["grad_enh"]
    rng = np.random.default_rng(1000 * B + T)
    spec = (rng.standard_normal((B, 257, T, 2)) * 0.3).astype(np.float32)
    gout = (rng.standard_normal((B, 257, T, 2)) * 0.1).astype(np.float32)
    return blob, spec, gout


# The bounds of tests/test_gpu_train_pinned.py: 2x the worst measured on the MI355X over its shapes (the bf16 rows:
# dns3 / rand B = 3 x T = 12, B = 8 x T = 251) and fusion masks (measured values in the comments).
# (blob rel-L2, rel-L2 of a tensor of >= 16 elements, of a smaller one, max|err| / max|g| of a near-zero truth,
#  max|err| / max|g| of a tensor of fewer than 16 elements instead of its rel-L2)
BOUNDS = {
    # 1.42e-4 (dns3 goldens; 7.1e-6 rand, 2.2e-5 B = 8 x T = 251) | 5.6e-4 en_convs.2.tra.depth_conv.weight |
    # 1.5e-3 en_convs.4.depth_act.weight (1 element) | 1.3e-6 en_convs.0.conv.bias
    "bf16": (3e-4, 1.2e-3, 3e-3, 3e-6, None),
    # the unpinnable bf16 rounding of every gradient hand-off dominates (the CPU stand-in measures the same noise,
    # tests/test_pinned_checker.py): 9.3e-3 | 9.2e-2 en_convs.2.point_bn1.weight (rand, 16 elements; BatchNorm weights /
    # biases sum dz over every position and cancel) | - | 5.6e-6 | 3.1e-3 gtcn1.blocks.0.act1.weight
    "bf16_grads": (1.5e-2, 0.2, None, 1.2e-5, 6e-3),
    # Storage "f32": 2x the worst measured on the MI355X over the 152 cases of
    # test_f32_train_step_per_unit_against_the_pinned_checker (dns3 / rand x four fusion masks x F32_SHAPES); the float32
    # port on the CPU sits at the same level or above (tests/test_pinned_checker.py).
    # The absolute class is by name here: the 46 conv biases in front of a BatchNorm (and a truth exactly 0); every
    # other tensor is held by rel-L2, the f32_cancelling ones by F32_CANCELLING.
    # 1.02e-6 (dns3 2 x 65, mask 0) | 5.4e-5 gtcn2.blocks.3.bn1.weight (rand 2 x 251) | 9.3e-4 en_convs.2.point_act.weight
    # (1 element, rand 1 x 1, mask 0; 8.2e-4 gtcn1.blocks.0.act1.weight, dns3 1 x 1; from B x T >= 12 on 3.1e-4, rand
    # 1 x 33) | 1.89e-6 en_convs.0.conv.bias (rand 2 x 251)
    "f32": (2e-6, 1.1e-4, 1.9e-3, 3.8e-6, None),
}
FWD_ADJ = 2.7e-3      # share of the elements of a stored tensor one bf16 step from the checker's value: 1.32e-3 (en4)
FWD_FAR = 2.2e-5      # share of all stored elements further apart: 1.1e-5
STATS = 1.2e-7        # running statistics after the step, max|err| / max|value| per tensor: 5.3e-8
OUT = 1.2e-7          # the enhanced spectrogram (spec x the pinned mask): 5.8e-8
# storage "f32"
# rel-L2 of the TCN's depthwise weights whose dilation >= T (f32_cancelling): 1.53e-3 gtcn1.blocks.3.conv2.weight (dns3
# 2 x 3, mask 1023; 1.34e-3 gtcn2.blocks.2.conv2.weight there, 9.7e-4 at 2 x 7; the float32 port on the CPU 2.1e-3)
F32_CANCELLING = 3.1e-3
FWD_REL = 1.3e-6      # a stored tensor against the checker's value, max|err| / max|stored|: 6.7e-7 (de_convs.1.depth_bn.y)
STATS_F32 = 1.15e-7   # running statistics after the step: 5.74e-8
OUT_F32 = 1.8e-7      # the enhanced spectrogram: 8.8e-8


def tap_names():
    ys = [n[:-len(".running_mean")] + ".y" for n, _, _ in param_table() if n.endswith(".running_mean")]
    return ys + [f"en{i}" for i in range(5)] + [f"tcn{i}" for i in range(8)] + ["gtcn1", "gtcn2"] + \
        [f"sum{i}" for i in range(5)] + [f"de{i}" for i in range(5)]


def read_taps(tr, fusions, clips=None):
    """Every stored tensor the trainer has a tap for, on the host (float64); the first `clips` clips only."""
    from gtcrn_micro_amd._lib import GtcrnError
    taps = {}
    for name in tap_names():
        try:
            v = tr.tap(name)
        except GtcrnError:
            continue                    # (a shared sum buffer holds only the last sum after the forward)
        taps[name] = (v if clips is None else v[:clips]).double().cpu()
    if "sum0" in taps and fusions & 2048:
        for name in SUM_MINUS_TAPS:     # stored only as sum - skip: the sums are pinned instead
            taps.pop(name, None)
    return taps


def assert_pinned_step(storage, blob_np, spec_np, gout_np, taps, grads, blob_after, out, what, scale=1.0, stats=STATS,
                       lost_frame=None):
    """The whole per-unit check of one HIP step against the pinned float64 checker; returns the gradient report.
    scale: the trainer's batch is the checker's tiled `scale` times (its gradient is `scale` x the checker's).
    Storage "f32" (scale and stats at their defaults): the fp32 bounds, the forward held as a relative error per stored
    tensor, the finer seeded bugs; lost_frame: the frame of clip 0 whose upstream gradient the lost-frame bug drops."""
    if storage == "f32":
        assert scale == 1.0 and stats == STATS
        fig = f32_figures(blob_np, spec_np, gout_np, taps, grads, blob_after, out, BOUNDS["f32"], F32_CANCELLING,
                          lost_frame, what)
        assert fig["fwd"][1] < FWD_REL, fig["fwd"]
        assert fig["out"] < OUT_F32 and fig["stats"] < STATS_F32, (fig["out"], fig["stats"])
        assert not fig["fails"], fig["fails"]
        # seeded unit bugs in the trainer's gradient: each is caught by the same check
        assert all(fig["caught"].values()), fig["caught"]
        return fig["rows"]
    gr = storage == "bf16_grads"
    mine, enh64, g64, b64 = pinned_truth(blob_np, spec_np, gout_np, taps, grad_round=gr)
    agree = forward_agreement(mine, {n: v.numpy() for n, v in taps.items()})
    n_all = sum(v.numel() for v in taps.values())
    far = sum(v[1] for v in agree.values()) / n_all
    w_adj = max(agree.items(), key=lambda kv: kv[1][0])
    e_out, stat_err = _out_and_stats(out, enh64, blob_after, b64)
    ga = np.asarray(grads, np.float64) / scale
    e_all, rows, fails = check_grads(ga, g64, *BOUNDS[storage])
    print(f"{what}: {len(taps)} pinned tensors; forward: worst adjacent share {w_adj[0]} {w_adj[1][0]:.2e}, further "
          f"apart {far:.1e}, output {e_out:.1e}, running statistics {stat_err:.1e}; gradient: {summary(e_all, rows)}")
    _print_worst(rows)
    assert w_adj[1][0] < FWD_ADJ and far < FWD_FAR, (w_adj, far)
    assert e_out < OUT and stat_err < stats, (e_out, stat_err)
    assert not fails, fails
    # seeded unit bugs in the trainer's gradient: each is caught by the same check
    for name, g in mutations(ga, g64):
        if storage == "bf16_grads" and name != "gtcn2.blocks.1.conv2.weight":
            continue                    # (under the noise of the unpinnable gradient roundings: held in "bf16")
        assert name in [f[0] for f in check_grads(g, g64, *BOUNDS[storage])[2]], name
    return rows


def _out_and_stats(out, enh64, blob_after, b64):
    e_out = float(np.abs(out - enh64).max() / np.abs(enh64).max())
    stat_err = 0.0
    for name, numel, off in param_table():
        if name.endswith("running_mean") or name.endswith("running_var"):
            t = b64[off:off + numel]
            stat_err = max(stat_err, float(np.abs(blob_after[off:off + numel] - t).max() / np.abs(t).max()))
    return e_out, stat_err


def _print_worst(rows):
    for r in sorted(rows, key=lambda r: -(r[3] if r[4] else r[2]))[:5]:
        print(f"    {r[0]} ({r[1]} el.): rel-L2 {r[2]:.2e}, max|err| {r[3]:.1e} of max|g|{' (near-zero truth)' if r[4] else ''}")


def _bt(spec_np):
    return spec_np.shape[0], spec_np.shape[2]


def conv_biases_before_bn():
    """The 46 conv biases in front of a train-mode BatchNorm, whose centring takes them out: true gradient exactly 0."""
    out = set()
    for n, _, _ in param_table():
        if n.endswith(".running_mean"):
            head, bn = n[:-len(".running_mean")].rsplit(".", 1)
            out.add(f"{head}.{bn.replace('bn', 'conv')}.bias")
    return out


def f32_cancelling(T):
    """The TCN's depthwise weights whose dilation d >= T: both earlier taps see only padding (gradient exactly 0), the
    unit is a per-channel scale in front of a train-mode BatchNorm, and the gradient of the tap that is left,
    sum dy x = (gamma / sigma) sum(dz z) eps / (var + eps), is what BatchNorm's eps leaves of a sum that would cancel
    to 0 without it: ~1e-3 of its terms, so float32 keeps three digits fewer of it than of any other tensor."""
    return {f"gtcn{g}.blocks.{k}.conv2.weight" for g in (1, 2) for k in range(4) if (1 << k) >= T}


def f32_figures(blob_np, spec_np, gout_np, taps, grads, blob_after, out, bounds, cancelling_bound, lost_frame, what):
    """Every figure of the fp32 check of one step (the HIP trainer's, or the float32 port's as its stand-in) against the
    float64 checker pinned to `taps`.  Held by rel-L2: every trainable tensor but the conv biases in front of a
    BatchNorm and tensors whose truth is exactly 0 (absolute bound); the f32_cancelling ones by a bound of their own."""
    B, T = _bt(spec_np)
    mine, enh64, g64, b64 = pinned_truth(blob_np, spec_np, gout_np, taps, storage="f32")
    fwd = forward_rel(mine, {n: np.asarray(v) for n, v in taps.items()})
    w_fwd = max(fwd.items(), key=lambda kv: kv[1])
    e_out, stat_err = _out_and_stats(out, enh64, blob_after, b64)
    ga = np.asarray(grads, np.float64)
    how = dict(abs_class=conv_biases_before_bn(), special={n: cancelling_bound for n in f32_cancelling(T)})
    e_all, rows, fails = check_grads(ga, g64, *bounds, **how)
    plain = [r for r in rows if r[0] not in how["special"]]
    canc = [r for r in rows if r[0] in how["special"]]
    print(f"{what}: {len(taps)} pinned tensors; forward: worst stored tensor {w_fwd[0]} {w_fwd[1]:.2e}, output "
          f"{e_out:.1e}, running statistics {stat_err:.1e}; gradient: {summary(e_all, plain)}; cancelling depthwise "
          f"weights (dilation >= T): {max((r[2] for r in canc), default=0.0):.2e}")
    _print_worst(rows)
    lost = None if lost_frame is None else lost_frame_gradient(blob_np, spec_np, gout_np, taps, lost_frame)
    caught = {name: rejected(name, check_grads(g, g64, *bounds, **how)[2]) for name, g in mutations_f32(ga, g64, lost)}
    return dict(blob=e_all, rows=rows, fails=fails, fwd=w_fwd, out=e_out, stats=stat_err, caught=caught,
                lost_share=None if lost is None else float(np.linalg.norm(lost) / np.linalg.norm(g64)))
