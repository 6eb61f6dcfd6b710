"""Unit-level checker of the bf16 train step: the float64 port pinned to the tensors the trainer stored.

TEST INFRASTRUCTURE ONLY, like everything under oracle/.
Without pins, one bf16 rounding flip early in the 46-unit chain moves the whole downstream forward, and even the same
bf16 network evaluated in fp32 and in float64 ends 0.2 .. 0.4 apart in gradient.  Pinned (TorchPort(pin=...)), every
unit of the float64 checker sees exactly the inputs the trainer's unit saw, so what is left between the two gradients is
the arithmetic of the units themselves -- small enough to catch a unit that is wrong by a few per cent.
"""
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


def record(blob, spec, grad_enh, dtype=torch.float32, grad_round=False):
    """The float32 stand-in for the device: its forward taps (every stored tensor by name) and its gradient."""
    taps = {}
    port = TorchPort(np.asarray(blob, np.float32).copy(), train=True, dtype=dtype, store="bf16", grad_round=grad_round)
    enh, grads = port.backward_from(spec, grad_enh, taps=taps)
    return taps, enh, grads, port.blob()


def pinned_truth(blob, spec, grad_enh, pins, grad_round=False):
    """The float64 checker pinned to `pins`: (its own pre-snap values of every stored tensor, forward output, gradient
    blob, blob after the step -- running statistics updated)."""
    taps = {}
    port = TorchPort(np.asarray(blob, np.float32).copy(), train=True, dtype=torch.float64, store="bf16", pin=pins,
                     grad_round=grad_round)
    enh, grads = port.backward_from(spec, grad_enh, taps=taps)
    return taps, enh, grads.astype(np.float64), _blob64(port)


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


def grad_report(got, truth):
    """Per trainable tensor with a gradient: (name, numel, rel-L2, max|err| / max|truth of the blob|, near-zero truth)."""
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
        near0 = float(np.abs(t).max()) < 1e-4 * gmax
        rows.append((name, numel, rel, ab, near0))
    return rows


def check_grads(got, truth, blob_bound, tensor_bound, small_bound, abs_bound, small_abs=None):
    """The pinned gradient check: blob rel-L2 <= blob_bound; per tensor rel-L2 <= tensor_bound (>= 16 elements) or
    small_bound (fewer: biases of the 2-/8-channel layers, PReLU slopes); tensors whose truth is ~0 instead
    max|err| <= abs_bound * max|truth|.  small_abs (instead of small_bound): the tensors of fewer than 16 elements are
    held by max|err| <= small_abs * max|truth| -- for the noise of unpinnable gradient roundings, which a scalar's
    rel-L2 does not average.  Returns (blob rel-L2, report rows, failures)."""
    got = np.asarray(got, np.float64)
    truth = np.asarray(truth, np.float64)
    e_all = float(np.linalg.norm(got - truth) / np.linalg.norm(truth))
    rows = grad_report(got, truth)
    fails = []
    if not e_all <= blob_bound:
        fails.append(("<blob>", e_all, blob_bound))
    for name, numel, rel, ab, near0 in rows:
        if near0:
            if not ab <= abs_bound:
                fails.append((name, ab, abs_bound))
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


def mutations(got, truth):
    """Seeded unit bugs, applied to a gradient blob: one BatchNorm weight vector x1.01, one PReLU slope x1.05 (the one
    with the largest true gradient), one depthwise-weight tap (all channels) zeroed."""
    tab = {n: (k, o) for n, k, o in param_table()}
    truth = np.asarray(truth, np.float64)
    out = []
    g = np.array(got, np.float64, copy=True)
    k, o = tab["gtcn1.blocks.2.bn2.weight"]
    g[o:o + k] *= 1.01
    out.append(("gtcn1.blocks.2.bn2.weight", g))
    slopes = [n for n, (k, _) in tab.items() if k == 1 and "act" in n.split(".")[-2]]
    slope = max(slopes, key=lambda n: abs(truth[tab[n][1]]))
    g = np.array(got, np.float64, copy=True)
    g[tab[slope][1]] *= 1.05
    out.append((slope, g))
    g = np.array(got, np.float64, copy=True)
    k, o = tab["gtcn2.blocks.1.conv2.weight"]          # (16, 1, 3, 1): tap 0 of every channel
    g[o:o + k].reshape(16, 3)[:, 0] = 0.0
    out.append(("gtcn2.blocks.1.conv2.weight", g))
    return out


# The bounds of tests/test_gpu_train_pinned.py: 2x the worst measured on the MI355X over its shapes (dns3 / rand
# B = 3 x T = 12, B = 8 x T = 251) and fusion masks (measured values in the comments).
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
}
FWD_ADJ = 2.7e-3      # share of the elements of a stored tensor one bf16 step from the checker's value: 1.32e-3 (en4)
FWD_FAR = 2.2e-5      # share of all stored elements further apart: 1.1e-5
STATS = 1.2e-7        # running statistics after the step, max|err| / max|value| per tensor: 5.3e-8
OUT = 1.2e-7          # the enhanced spectrogram (spec x the pinned mask): 5.8e-8


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


def assert_pinned_step(storage, blob_np, spec_np, gout_np, taps, grads, blob_after, out, what, scale=1.0, stats=STATS):
    """The whole per-unit check of one HIP step against the pinned float64 checker; returns the gradient report.
    scale: the trainer's batch is the checker's tiled `scale` times (its gradient is `scale` x the checker's)."""
    gr = storage == "bf16_grads"
    mine, enh64, g64, b64 = pinned_truth(blob_np, spec_np, gout_np, taps, grad_round=gr)
    agree = forward_agreement(mine, {n: v.numpy() for n, v in taps.items()})
    n_all = sum(v.numel() for v in taps.values())
    far = sum(v[1] for v in agree.values()) / n_all
    w_adj = max(agree.items(), key=lambda kv: kv[1][0])
    e_out = float(np.abs(out - enh64).max() / np.abs(enh64).max())
    stat_err = 0.0
    for name, numel, off in param_table():
        if name.endswith("running_mean") or name.endswith("running_var"):
            t = b64[off:off + numel]
            stat_err = max(stat_err, float(np.abs(blob_after[off:off + numel] - t).max() / np.abs(t).max()))
    ga = np.asarray(grads, np.float64) / scale
    e_all, rows, fails = check_grads(ga, g64, *BOUNDS[storage])
    print(f"{what}: {len(taps)} pinned tensors; forward: worst adjacent share {w_adj[0]} {w_adj[1][0]:.2e}, further "
          f"apart {far:.1e}, output {e_out:.1e}, running statistics {stat_err:.1e}; gradient: {summary(e_all, rows)}")
    for r in sorted(rows, key=lambda r: -(r[3] if r[4] else r[2]))[:5]:
        print(f"    {r[0]} ({r[1]} el.): rel-L2 {r[2]:.2e}, max|err| {r[3]:.1e} of max|g|{' (near-zero truth)' if r[4] else ''}")
    assert w_adj[1][0] < FWD_ADJ and far < FWD_FAR, (w_adj, far)
    assert e_out < OUT and stat_err < stats, (e_out, stat_err)
    assert not fails, fails
    # seeded unit bugs in the trainer's gradient: each is caught by the same check
    for name, g in mutations(ga, g64):
        if storage == "bf16_grads" and name != "gtcn2.blocks.1.conv2.weight":
            continue                    # (under the noise of the unpinnable gradient roundings: held in "bf16")
        assert name in [f[0] for f in check_grads(g, g64, *BOUNDS[storage])[2]], name
    return rows
