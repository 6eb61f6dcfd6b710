"""Inputs, references and acceptance function for the fused HybridLoss (gtcrn_train_loss / gtcrn_train_loss_strided),
shared by tests/test_hybrid_loss_checker.py (CPU) and tests/test_gpu_hybrid_loss.py (GPU).

Three statements of loss.py:30-71 live here, all on the CPU:
  loss_f64           torch float64 with autograd: the reference every result is held against
  loss_f32           oracle/torch_port.py's TorchPort.hybrid_loss in float32 with autograd: the floor
  loss_kernel_order  float32 in the kernels' own order (closed-form gradient, three sums per utterance, A yp + B yt,
                     envelope division, iSTFT adjoint), with switches that seed one bug each (BUGS)
See `accept` for the rule; the measured floors and ratios stand next to K_VALUE / K_GRAD."""
import functools
import math

import numpy as np
import torch

# The margins of `accept`: a statistic may be at most K times its floor (loss_f32 against loss_f64, same case, max over
# the seeds).  All figures below are statistic / floor; the per-case table is in tests/reports/README.md.
#   floors (CPU)    value 0.6e-7 .. 3e-7 (at least one float32 rounding of the value, see `reference`), near_80 2.5e-6;
#                   gradient statistics 1.6e-7 .. 7e-6 on unrelated inputs (an utterance whose prediction is nearly
#                   orthogonal to its target has an ill-conditioned <yt, yp>: that draw sets the floor, and the spread
#                   between cases of one kind is a factor of 20), 7e-5 over 1024 utterances of one hop, and 2e-5 ..
#                   3e-3 at near_40 .. near_80; near_100 / near_120 reach 0.02 .. 0.3 and identical 3 .. 5: float32
#                   cannot define the residual's direction there and the rule holds the value and finiteness only
#   kernel order (CPU, loss_kernel_order, every case x seed): value <= 1.2, gradient <= 6.7 (random-B3-T9, seed 1,
#                   utterance 1: <yt, yp> = 9.5e-4 against |yt| |yp| = 2.0, both float32 evaluations carry an absolute
#                   error of 3e-9 in it and the torch one happens to land closer)
#   kernels (MI355X), every case x seed x layout: value <= 1.94 (loud), gradient <= 6.68 (loud), 5.37 (silent_target),
#                   3.58 (zero_bins), 2.66 (tiny_bins); everything else <= 1.3
#   seeded bugs (BUGS), best ratio on the case that rejects each most clearly: 1e5 .. 8e7 on unrelated inputs; the
#                   closest call the rule has to make is the residual from float32-rounded products (the kernels'
#                   arithmetic before k_sisnr_sums formed its products in double), value / floor 37 at near_40, 370 at
#                   near_60, 3.9e3 at near_80 here and 6 / 468 / 5.1e3 / 3.4e4 / 6.2e4 at near_40 .. near_120 on the
#                   MI355X -- the first bug escapes at K_VALUE > 5e3 and K_GRAD > 1e5
# K = twice the kernels' worst ratio, rounded up to one significant digit (1.94 -> 4, 6.68 -> 20): the room for another
# draw of the rounding on other seeds and for the floor's own spread.
K_VALUE = 4.0
K_GRAD = 20.0

BAND = 16          # bins per band of grad_band (17 bands: the last holds the Nyquist bin alone)
BUGS = ("no_eps_mag", "no_eps_proj", "f32_products", "lambda_swapped", "mean_2N", "coef_swap", "no_1_over_B", "hann",
        "no_cross", "exp069")


KINDS = ("random", "zero_bins", "tiny_bins", "silent_target", "silent_pred", "both_silent", "scale", "near", "identical")


def window32():
    """The kernels' stated window: gtcrn_make_window(0), 512 float32 values."""
    from gtcrn_micro_amd import make_window
    return np.asarray(make_window(0), np.float32)


# ------------------------------------------------------------------------------------------------------------- cases
class Case:
    """`seeds` inputs of one kind and shape; the floors are the max over them.  layout: which of pred / true the GPU test
    hands over frame-major ((B,T,257,2) memory viewed as (B,257,T,2)); the values do not depend on it."""

    def __init__(self, name, kind, B, T, seeds=(0, 1, 2), param=None, layout=""):
        self.name, self.kind, self.B, self.T, self.seeds = name, kind, B, T, tuple(seeds)
        self.param, self.layout = param, layout

    def __repr__(self):
        return self.name

    def input(self, seed):
        """(pred, true): float32 (B,257,T,2)."""
        rng = np.random.default_rng([seed, self.B, self.T, KINDS.index(self.kind)])
        shape = (self.B, 257, self.T, 2)
        pred = (rng.standard_normal(shape) * 0.5).astype(np.float32)
        true = (rng.standard_normal(shape) * 0.5).astype(np.float32)
        k = self.kind
        if k == "zero_bins":
            pred[:, 0::3] = 0.0
            true[:, 1::3] = 0.0
            pred[:, :, self.T // 2] = 0.0
            true[:, :, self.T // 2] = 0.0
        elif k == "tiny_bins":
            pred[rng.random(shape[:3]) < 0.5] *= np.float32(1e-6)
            true[rng.random(shape[:3]) < 0.5] *= np.float32(1e-6)
        elif k == "silent_target":
            true[1] = 0.0
        elif k == "silent_pred":
            pred[2] = 0.0
        elif k == "both_silent":
            pred[:] = 0.0
            true[:] = 0.0
        elif k == "scale":
            pred *= np.float32(self.param)
            true *= np.float32(self.param)
        elif k == "near":
            noise = rng.standard_normal(shape) * 0.5 * 10.0 ** (-self.param / 20.0)
            pred = (true.astype(np.float64) + noise).astype(np.float32)
        elif k == "identical":
            pred = true.copy()
        else:
            assert k == "random", k
        return pred, true


def _cases():
    out = [Case("random-B1-T2", "random", 1, 2), Case("random-B3-T9", "random", 3, 9),
           Case("random-B2-T17", "random", 2, 17)]
    for kind in ("zero_bins", "tiny_bins", "silent_target", "silent_pred"):
        out.append(Case(kind, kind, 3, 9))
    out.append(Case("both_silent", "both_silent", 2, 4))
    out.append(Case("loud", "scale", 3, 9, param=60.0))
    out.append(Case("faint", "scale", 3, 9, param=2e-4))
    for db in (40, 60, 80, 100, 120):
        out.append(Case(f"near_{db}", "near", 3, 9, param=float(db)))
    out.append(Case("identical", "identical", 3, 9))
    for layout in ("pred", "true", "both"):
        out.append(Case(f"random-B3-T9-fmaj-{layout}", "random", 3, 9, layout=layout))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
# the one-launch limit (one utterance per thread of k_sisnr_coef's only block) and the first size HybridLoss chunks
BIG_CASES = (Case("random-B1024-T2", "random", 1024, 2, seeds=(0,)), Case("random-B1025-T2", "random", 1025, 2, seeds=(0,)))


# ------------------------------------------------------------------------------------------------- the three statements
def _torch_hybrid(pred, true, win):
    """loss.py:30-71 as torch ops in the dtype of its arguments; the SI-SNR energies as sums of squares, so that autograd
    is defined at a zero waveform.  Returns (loss, per-utterance SI-SNR terms)."""
    pr, pi, tr, ti = pred[..., 0], pred[..., 1], true[..., 0], true[..., 1]
    pm = torch.sqrt(pr ** 2 + pi ** 2 + 1e-12)
    tm = torch.sqrt(tr ** 2 + ti ** 2 + 1e-12)
    mse = torch.nn.functional.mse_loss
    ri = mse(pr / pm ** 0.7, tr / tm ** 0.7) + mse(pi / pm ** 0.7, ti / tm ** 0.7)
    mag = mse(pm ** 0.3, tm ** 0.3)
    yp = torch.istft(torch.complex(pr, pi), 512, 256, 512, window=win)
    yt = torch.istft(torch.complex(tr, ti), 512, 256, 512, window=win)
    s = torch.sum(yt * yp, -1, keepdim=True) * yt / (torch.sum(yt ** 2, -1, keepdim=True) + 1e-8)
    terms = -torch.log10(torch.sum(s ** 2, -1) / (torch.sum((yp - s) ** 2, -1) + 1e-8) + 1e-8)
    return 30 * ri + 70 * mag + terms.mean(), terms


def loss_f64(pred, true):
    """The reference: float64 on the CPU, the window the kernels' 512 float32 values widened to double.
    Returns (value, gradient w.r.t. pred (B,257,T,2) float64, per-utterance SI-SNR terms (B,) float64)."""
    p = torch.from_numpy(np.asarray(pred, np.float64)).requires_grad_(True)
    t = torch.from_numpy(np.asarray(true, np.float64))
    loss, terms = _torch_hybrid(p, t, torch.from_numpy(window32().astype(np.float64)))
    loss.backward()
    return float(loss.detach()), p.grad.numpy(), terms.detach().numpy()


def loss_f32(pred, true):
    """The floor: the reference's own formulation at the reference's own precision (TorchPort.hybrid_loss, float32, CPU,
    autograd).  Returns (value, gradient float32)."""
    from oracle.torch_port import TorchPort
    p = torch.from_numpy(np.array(pred, np.float32)).requires_grad_(True)
    loss = TorchPort.hybrid_loss(p, torch.from_numpy(np.array(true, np.float32)))
    loss.backward()
    return float(loss.detach()), p.grad.numpy()


def _istft32(spec, win, env):
    """k_istft: c2r of every frame (1/512), * win, overlap-add, / envelope, 256 samples trimmed at both ends."""
    z = torch.complex(spec[..., 0], spec[..., 1]).permute(0, 2, 1)               # (B,T,257)
    fr = torch.fft.irfft(z, n=512, dim=-1) * win                                  # (B,T,512)
    acc = fr[:, :-1, 256:] + fr[:, 1:, :256]                                      # block j: frame j's tail + frame j+1's head
    return (acc / env).reshape(spec.shape[0], -1)                                 # (env > 1e-11 for either window)


def _istft_adjoint32(gwave, T, win):
    """k_stft<true>: frames of the zero-padded signal, * win, r2c, every bin scaled by c_k / 512 (c_k = 2 except DC and
    Nyquist, whose imaginary parts the c2r transform never read)."""
    B = gwave.shape[0]
    x = torch.nn.functional.pad(gwave, (256, 256)).reshape(B, T + 1, 256)
    fr = torch.cat([x[:, :-1], x[:, 1:]], dim=-1) * win                           # (B,T,512)
    z = torch.fft.rfft(fr, dim=-1)                                                # (B,T,257)
    ck = torch.full((257,), 2.0 / 512.0, dtype=torch.float32)
    ck[0] = ck[256] = 1.0 / 512.0
    g = torch.stack([z.real * ck, z.imag * ck], dim=-1)
    g[:, :, 0, 1] = 0.0
    g[:, :, 256, 1] = 0.0
    return g.permute(0, 2, 1, 3)                                                  # (B,257,T,2)


def loss_kernel_order(pred, true, bug=None):
    """What the kernels compute, in float32 and in their order, on the CPU: k_hloss_spec (value in double sums of float32
    terms, closed-form gradient), k_istft twice, k_sisnr_sums (double sums of exact products), k_sisnr_coef (double),
    k_sisnr_gwave, the iSTFT adjoint added to the spectral gradient.  `bug`: one of BUGS, seeded into that order.
    Returns (value, gradient float32 (B,257,T,2), per-utterance terms float64)."""
    assert bug is None or bug in BUGS, bug
    f32 = np.float32
    p = torch.from_numpy(np.array(pred, f32))
    q = torch.from_numpy(np.array(true, f32))
    B, _, T, _ = p.shape
    N = B * 257 * T * (2 if bug == "mean_2N" else 1)
    lam_ri, lam_mag = (70.0, 30.0) if bug == "lambda_swapped" else (30.0, 70.0)
    kri, kmag = f32(2 * lam_ri) / f32(N), f32(2 * lam_mag) / f32(N)
    eps_mag = f32(0.0 if bug == "no_eps_mag" else 1e-12)
    e_ri = f32(-0.69 if bug == "exp069" else -0.7)
    px, py, qx, qy = p[..., 0], p[..., 1], q[..., 0], q[..., 1]
    pm2, tm2 = px * px + py * py + eps_mag, qx * qx + qy * qy + eps_mag
    lp, lt = 0.5 * torch.log2(pm2), 0.5 * torch.log2(tm2)
    u, ut = torch.exp2(e_ri * lp), torch.exp2(e_ri * lt)
    c, ct = torch.exp2(f32(0.3) * lp), torch.exp2(f32(0.3) * lt)
    da, db, dc = px * u - qx * ut, py * u - qy * ut, c - ct
    sri = float((da * da + db * db).double().sum())
    smag = float((dc * dc).double().sum())
    inv = 1.0 / pm2
    w = f32(0.7) * u * inv
    a_r, a_i, b_i = u - w * px * px, -w * px * py, u - w * py * py
    if bug == "no_cross":
        a_i = torch.zeros_like(a_i)
    cw = f32(0.3) * c * inv
    grad = torch.stack([kri * (da * a_r + db * a_i) + kmag * dc * cw * px,
                        kri * (da * a_i + db * b_i) + kmag * dc * cw * py], dim=-1)
    # SI-SNR of the two waveforms
    win = torch.from_numpy(window32())
    if bug == "hann":
        win = win * win
    env = win[256:] * win[256:] + win[:256] * win[:256]
    yp, yt = _istft32(p, win, env), _istft32(q, win, env)
    if bug == "f32_products":
        dot, ett, epp = ((a * b).double().sum(-1).numpy() for a, b in ((yp, yt), (yt, yt), (yp, yp)))
    else:
        ypd, ytd = yp.double(), yt.double()
        dot, ett, epp = ((a * b).sum(-1).numpy() for a, b in ((ypd, ytd), (ytd, ytd), (ypd, ypd)))
    eps = 1e-8
    eps_proj = 0.0 if bug == "no_eps_proj" else eps
    with np.errstate(all="ignore"):
        al = dot / (ett + eps_proj)
        num = al * al * ett
        den = epp - 2.0 * al * dot + al * al * ett + eps
        r = num / den
        terms = -np.log10(r + eps)
        c0 = (1.0 if bug == "no_1_over_B" else 1.0 / B) * (-1.0 / ((r + eps) * 2.302585092994046))
        kap, eta = ett / (ett + eps_proj), (dot - al * ett) / (ett + eps_proj)
        cA = (c0 * (-2.0 * num / (den * den))).astype(f32)
        cB = (c0 * (2.0 * al * kap / den + 2.0 * num * (al + eta) / (den * den))).astype(f32)
    if bug == "coef_swap":
        idx = np.array([b ^ 1 if (b ^ 1) < B else b for b in range(B)])
        cA, cB = cA[idx], cB[idx]
    gwave = (torch.from_numpy(cA)[:, None] * yp + torch.from_numpy(cB)[:, None] * yt) / env.repeat(T - 1)
    grad = grad + _istft_adjoint32(gwave, T, win)
    value = f32(lam_ri * sri / N + lam_mag * smag / N + terms.sum() / B)
    return float(value), grad.numpy(), terms


# ------------------------------------------------------------------------------------------------------------- the rule
STATS = ("value", "grad_l2", "grad_band", "grad_max")


def _ratio(num, den):
    return num / den if den > 0 else (0.0 if num == 0 else math.inf)


def stats(value, grad, ref_value, ref_grad):
    """(value, grad_l2, grad_band, grad_max) of a result against the float64 reference:
      value      |L - L64| / max(|L64|, 1)
      grad_l2    per utterance ||g - g64|| / ||g64||, the worst utterance
      grad_band  the same ratio per utterance and band of 16 bins, the worst band (bands whose ||g64|| is 0 are skipped)
      grad_max   per utterance max|g - g64| / max|g64|, the worst
    An utterance whose g64 is all zero counts 0 when g is too and inf otherwise.  A non-finite input gives inf."""
    g, r = np.asarray(grad, np.float64), np.asarray(ref_grad, np.float64)
    assert g.shape == r.shape, (g.shape, r.shape)
    if not (np.isfinite(value) and np.isfinite(g).all()):
        return (math.inf,) * 4
    sv = abs(float(value) - ref_value) / max(abs(ref_value), 1.0)
    l2 = band = mx = 0.0
    for b in range(g.shape[0]):
        d = g[b] - r[b]
        l2 = max(l2, _ratio(np.linalg.norm(d), np.linalg.norm(r[b])))
        mx = max(mx, _ratio(np.abs(d).max(), np.abs(r[b]).max()))
        for f in range(0, 257, BAND):
            nr = np.linalg.norm(r[b, f:f + BAND])
            if nr > 0:
                band = max(band, np.linalg.norm(d[f:f + BAND]) / nr)
    return sv, float(l2), float(band), float(mx)


@functools.lru_cache(maxsize=None)
def reference(case):
    """({seed: (pred, true, L64, g64, terms64)}, floors): the floors are the four statistics of loss_f32 against
    loss_f64, max over the case's seeds.  Computed once per case, shared, never written to.

    The value floor is at least one float32 rounding of the reference value, 2^-24 |L64| / max(|L64|, 1): the loss
    leaves the kernels as a float, and where loss_f32 happens to land on the float nearest to L64 (both_silent: exactly
    8) the measured figure says nothing about how close another float32 evaluation can be expected to come."""
    per_seed, rows = {}, []
    for s in case.seeds:
        pred, true = case.input(s)
        L64, g64, t64 = loss_f64(pred, true)
        L32, g32 = loss_f32(pred, true)
        st = list(stats(L32, g32, L64, g64))
        st[0] = max(st[0], 2.0 ** -24 * abs(L64) / max(abs(L64), 1.0))
        rows.append(st)
        for a in (pred, true, g64, t64):
            a.setflags(write=False)
        per_seed[s] = (pred, true, L64, g64, t64)
    return per_seed, tuple(max(v) for v in zip(*rows))


def gradient_defined(case):
    """False where float32 cannot define the gradient (pred == true, or a gradient floor above 0.5: the residual
    yp - s is rounding noise): the gradient is then only required to be finite."""
    return case.kind != "identical" and max(reference(case)[1][1:]) <= 0.5


def accept(got_value, got_grad, case, seed=None, terms=None, k_value=K_VALUE, k_grad=K_GRAD):
    """Hold one result (loss value, gradient w.r.t. pred, optionally the per-utterance SI-SNR terms) for input `seed` of
    `case` against loss_f64.  Returns (ok, stats, ratios to the floors, reasons for a rejection).

    Each statistic of `stats` may be at most K times its floor (k_value for the value, k_grad for the three gradient
    statistics); the floors come from `reference` at test time and nothing of the kernels' is in them.  A floor of 0
    demands equality.  On top of that, as conditions and not measurements:
      * value and gradient are finite, in every case;
      * both_silent: |L - 8| <= 1e-6 and the gradient is exactly zero;
      * silent_target / silent_pred: the silent utterance's term is 8 within 1e-6 (where `terms` is given);
      * where the gradient is not defined in float32 (`gradient_defined`), it only has to be finite."""
    seed = case.seeds[0] if seed is None else seed
    per_seed, floors = reference(case)
    pred, true, L64, g64, t64 = per_seed[seed]
    g = np.asarray(got_grad)
    why = []
    if not np.isfinite(got_value):
        why.append(f"value {got_value}")
    if not np.isfinite(g).all():
        why.append("gradient not finite")
    s = stats(got_value, g, L64, g64)
    ratios = tuple(_ratio(a, f) for a, f in zip(s, floors))
    ks = (k_value, k_grad, k_grad, k_grad)
    held = (0,) if not gradient_defined(case) else (0, 1, 2, 3)
    for i in held:
        if not s[i] <= ks[i] * floors[i]:
            why.append(f"{STATS[i]} {s[i]:.3e} > {ks[i]:g} x floor {floors[i]:.3e}")
    if case.kind == "both_silent":
        if not abs(got_value - 8.0) <= 1e-6:
            why.append(f"both silent: value {got_value!r} is not 8")
        if np.any(g != 0):
            why.append("both silent: gradient not exactly zero")
    if terms is not None and case.kind in ("silent_target", "silent_pred"):
        b = 1 if case.kind == "silent_target" else 2
        if not abs(float(np.asarray(terms)[b]) - 8.0) <= 1e-6:
            why.append(f"silent utterance {b}: term {np.asarray(terms)[b]!r} is not 8")
    return not why, s, ratios, why
