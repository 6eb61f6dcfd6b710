"""Reference, floor and acceptance function for gtcrn_clip_adam_step (k_grad_sqsum + k_adam_flat), shared by
tests/test_clip_adam_checker.py (CPU) and tests/test_gpu_clip_adam.py (GPU).

clip_adam_f64 states torch.nn.utils.clip_grad_norm_ + torch.optim.Adam.step() (train.py:282-285) in numpy float64;
clip_adam_f32 is those two torch calls themselves in float32 on the CPU: the floor.  Same construction as
tests/hybrid_loss_checker.py: a statistic of the kernel against float64 may be at most K_ADAM times the same statistic of
the floor."""
import functools

import numpy as np

# floors (CPU): norm, coefficient, gradient 6e-8 .. 9e-8, moments 6e-8 .. 2e-7 (1e-6 for exp_avg at n = 1), update
#               5e-6 .. 4e-5 (the update is lr-sized and is read off a parameter of size 1: one rounding of the parameter)
# kernels (MI355X), every scenario x both calls, statistic / floor: norm <= 0.96, coefficient <= 0.23, gradient <= 1.0,
#               exp_avg <= 1.42, exp_avg_sq <= 1.41, update <= 1.0.  Twice the worst, rounded up to one digit:
K_ADAM = 3.0

STATS = ("norm", "coef", "grad", "exp_avg", "exp_avg_sq", "update")
LR, BETAS, EPS = 3e-3, (0.9, 0.999), 1e-8


class Scenario:
    def __init__(self, name, n, max_norm=3.0, wd=0.0, step=1, grad_scale=10.0, warm=False):
        self.name, self.n, self.max_norm, self.wd, self.step = name, n, max_norm, wd, step
        self.grad_scale, self.warm = grad_scale, warm

    def __repr__(self):
        return self.name

    def input(self):
        """(params, [gradient of call 1, of call 2], exp_avg, exp_avg_sq, mask): float32 arrays of n elements.  About a
        third of the elements are masked out (buffers), none at n = 1; warm: moments as after many steps."""
        rng = np.random.default_rng([self.n, self.step, int(self.max_norm > 0)])
        f = np.float32
        p = rng.standard_normal(self.n).astype(f)
        grads = [(rng.standard_normal(self.n) * self.grad_scale).astype(f) for _ in range(2)]
        mask = (rng.random(self.n) < 0.65).astype(f) if self.n > 1 else np.ones(1, f)
        if self.warm:
            m, v = (rng.standard_normal(self.n) * 0.1).astype(f), (rng.random(self.n) * 0.02 + 1e-4).astype(f)
        else:
            m, v = np.zeros(self.n, f), np.zeros(self.n, f)
        return p, grads, m, v, mask


# sizes: a single element, a partial / full / just-over single workgroup of 256 (with one workgroup the first arriver is
# also the last), four workgroups with a partial last one
SCENARIOS = [Scenario(f"n{n}", n) for n in (1, 255, 256, 257, 1000)] + [
    Scenario("n1000-not-clipped", 1000, grad_scale=1e-3),
    Scenario("n1000-max_norm-0", 1000, max_norm=0.0),
    Scenario("n1000-max_norm-negative", 1000, max_norm=-1.0),
    Scenario("n257-zero-gradient-wd", 257, wd=1e-2, grad_scale=0.0),
    Scenario("n1000-wd", 1000, wd=1e-2),
    Scenario("n1000-step-10000", 1000, step=10000, warm=True),
]


def clip_adam_f64(p, g, m, v, mask, step, max_norm, wd, lr=LR, betas=BETAS, eps=EPS):
    """One call in float64: (params, gradient as clip_grad_norm_ leaves it, exp_avg, exp_avg_sq, total norm, clip
    coefficient).  Elements with mask == 0 do not count in the norm and do not move."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    on = np.asarray(mask) != 0
    norm = float(np.sqrt(np.sum(g[on] ** 2)))
    coef = min(max_norm / (norm + 1e-6), 1.0) if max_norm > 0 else 1.0
    g2 = np.where(on, g * coef, g)
    ge = g2 + wd * p
    m2 = m + (ge - m) * (1.0 - betas[0])
    v2 = v * betas[1] + (1.0 - betas[1]) * ge * ge
    bc1, bc2 = 1.0 - betas[0] ** step, 1.0 - betas[1] ** step
    p2 = p - (lr / bc1) * m2 / (np.sqrt(v2) / np.sqrt(bc2) + eps)
    return np.where(on, p2, p), g2, np.where(on, m2, m), np.where(on, v2, v), norm, coef


def clip_adam_f32(p, g, m, v, mask, step, max_norm, wd, lr=LR, betas=BETAS, eps=EPS):
    """The same call as torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in float32 on the CPU (masked-out elements
    carry a zero gradient there and are put back afterwards: torch moves them under weight decay)."""
    import torch
    on = np.asarray(mask) != 0
    q = torch.nn.Parameter(torch.from_numpy(np.array(p, np.float32)))
    q.grad = torch.from_numpy(np.where(on, g, 0).astype(np.float32))
    opt = torch.optim.Adam([q], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(np.array(m, np.float32)),
                    "exp_avg_sq": torch.from_numpy(np.array(v, np.float32))}
    if max_norm > 0:
        norm = float(torch.nn.utils.clip_grad_norm_([q], max_norm))
        coef = float(torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (torch.tensor(norm, dtype=torch.float32) + 1e-6),
                                 max=1.0))
    else:
        norm, coef = float(q.grad.norm()), 1.0
    opt.step()
    st = opt.state[q]
    return (np.where(on, q.detach().numpy(), p), np.where(on, q.grad.numpy(), g), np.where(on, st["exp_avg"].numpy(), m),
            np.where(on, st["exp_avg_sq"].numpy(), v), norm, coef)


def stats(got, ref, p_before):
    """Six statistics of one call's results (params, grad, exp_avg, exp_avg_sq, norm, coef) against float64: the norm
    relative, the coefficient absolute, each array as max|x - x64| / max|x64|, the parameters as their UPDATE
    (p - p_before: the update is lr-sized, the parameter itself would hide it).  An all-zero reference counts 0 when the
    result is zero too and inf otherwise."""
    def rel(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        d, s = float(np.abs(a - b).max()), float(np.abs(b).max())
        return d / s if s > 0 else (0.0 if d == 0 else float("inf"))
    p0 = np.asarray(p_before, np.float64)
    return (rel(got[4], ref[4]), abs(got[5] - ref[5]), rel(got[1], ref[1]), rel(got[2], ref[2]), rel(got[3], ref[3]),
            rel(np.asarray(got[0], np.float64) - p0, ref[0] - p0))


@functools.lru_cache(maxsize=None)
def reference(sc):
    """Two calls back to back (steps `step` and `step + 1`, a fresh gradient each), each continuing from the float64
    state: ([(inputs of the call, float64 results)], floors).  The floors are the statistics of clip_adam_f32 on the same
    inputs -- the float64 state rounded to float32 -- max over the two calls, and at least one float32 rounding (2^-24):
    every statistic is relative to the largest element, which a float result cannot hold more closely, and at n = 1 the
    float32 evaluation lands on the nearest float by luck."""
    p, grads, m, v, mask = sc.input()
    calls, rows = [], []
    for k, g in enumerate(grads):
        args = tuple(np.asarray(a, np.float32) for a in (p, g, m, v))
        ref = clip_adam_f64(*args, mask, sc.step + k, sc.max_norm, sc.wd)
        f32 = clip_adam_f32(*args, mask, sc.step + k, sc.max_norm, sc.wd)
        rows.append(stats(f32, ref, args[0]))
        calls.append((args + (mask,), ref))
        p, m, v = ref[0], ref[2], ref[3]
    return calls, tuple(max(max(c), 2.0 ** -24) for c in zip(*rows))


def accept(got, sc, call, k=K_ADAM):
    """Hold one call's results against float64: (ok, stats, ratios to the floors, reasons)."""
    calls, floors = reference(sc)
    args, ref = calls[call]
    why = [f"{name} not finite" for name, a in zip(("params", "grad", "exp_avg", "exp_avg_sq", "norm", "coef"), got)
           if not np.isfinite(np.asarray(a)).all()]
    s = stats(got, ref, args[0])
    ratios = tuple(a / f for a, f in zip(s, floors))
    why += [f"{n} {a:.3e} > {k:g} x floor {f:.3e}" for n, a, f in zip(STATS, s, floors) if not a <= k * f]
    off = args[4] == 0
    if not (np.array_equal(np.asarray(got[0])[off], args[0][off]) and np.array_equal(np.asarray(got[1])[off], args[1][off])
            and np.array_equal(np.asarray(got[2])[off], args[2][off]) and np.array_equal(np.asarray(got[3])[off], args[3][off])):
        why.append("a masked-out element moved")
    return not why, s, ratios, why
