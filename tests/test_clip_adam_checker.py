"""The float64 statement of clip_grad_norm_ + Adam (tests/clip_adam_checker.py) against torch itself, on the CPU."""
import numpy as np
import pytest

import clip_adam_checker as A

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("sc", A.SCENARIOS, ids=repr)
def test_f64_statement_is_torch_adam_in_double(sc):
    """clip_adam_f64 against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on float64 tensors, all elements
    trainable: the same formulas in the same precision, so the distance is a few double roundings."""
    p, grads, m, v, _ = sc.input()
    ones = np.ones(sc.n, np.float32)
    q = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
    opt = torch.optim.Adam([q], lr=A.LR, betas=A.BETAS, eps=A.EPS, weight_decay=sc.wd)
    opt.state[q] = {"step": torch.tensor(float(sc.step - 1), dtype=torch.float64),
                    "exp_avg": torch.from_numpy(m.astype(np.float64)), "exp_avg_sq": torch.from_numpy(v.astype(np.float64))}
    q.grad = torch.from_numpy(grads[0].astype(np.float64))
    norm = float(torch.nn.utils.clip_grad_norm_([q], sc.max_norm)) if sc.max_norm > 0 else float(q.grad.norm())
    opt.step()
    got = clip = A.clip_adam_f64(p, grads[0], m, v, ones, sc.step, sc.max_norm, sc.wd)
    assert abs(got[4] - norm) <= 1e-14 * max(norm, 1.0)
    for mine, theirs in ((got[0], q.detach()), (clip[1], q.grad), (got[2], opt.state[q]["exp_avg"]),
                         (got[3], opt.state[q]["exp_avg_sq"])):
        assert np.abs(mine - theirs.numpy()).max() <= 1e-13 * max(np.abs(mine).max(), 1.0)


def test_floor_is_accepted_and_a_wrong_step_is_not():
    """The float32 evaluation passes its own rule at K = 1 by construction; a bias correction from the wrong step, a
    norm that counts the masked-out elements and a missing clip are each rejected at K_ADAM."""
    for sc in A.SCENARIOS:
        calls, floors = A.reference(sc)
        print(f"{sc.name:26s} floors " + " ".join(f"{f:.2e}" for f in floors))
        for k, (args, _) in enumerate(calls):
            assert A.accept(A.clip_adam_f32(*args[:4], args[4], sc.step + k, sc.max_norm, sc.wd), sc, k, k=1.0)[0]
    sc = A.SCENARIOS[4]
    args, _ = A.reference(sc)[0][0]
    assert not A.accept(A.clip_adam_f32(*args[:4], args[4], sc.step + 1, sc.max_norm, sc.wd), sc, 0)[0]
    assert not A.accept(A.clip_adam_f32(*args[:4], np.ones_like(args[4]), sc.step, sc.max_norm, sc.wd), sc, 0)[0]
    assert not A.accept(A.clip_adam_f32(*args[:4], args[4], sc.step, 0.0, sc.wd), sc, 0)[0]
