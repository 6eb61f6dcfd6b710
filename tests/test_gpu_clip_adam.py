"""gtcrn_clip_adam_step (k_grad_sqsum + k_adam_flat) against a float64 numpy statement of clip_grad_norm_ + Adam, under
the rule of tests/clip_adam_checker.py: sizes round one workgroup of 256, no clipping, an all-zero gradient, a late step,
and two calls back to back on one workspace.  Run with -s to print the kernels' ratios to the floors."""
import numpy as np
import pytest

import clip_adam_checker as A

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sc", A.SCENARIOS, ids=repr)
def test_clip_adam_kernels_are_accepted(sc):
    import torch
    from gtcrn_micro_amd import _lib
    calls, floors = A.reference(sc)
    ws = _lib.clip_adam_workspace("cuda", sc.n)         # one workspace for both calls: the first leaves its ticket at zero
    worst = (0.0,) * 6
    for k, (args, ref) in enumerate(calls):
        p, g, m, v, mask = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args)
        out = torch.full((2,), float("nan"), device="cuda")
        _lib.clip_adam_step(p, g, m, v, mask, sc.step + k, A.LR, A.BETAS, A.EPS, sc.wd, sc.max_norm, out, ws)
        assert int(ws.view(torch.int32)[0]) == 0, "the last-workgroup ticket was not put back"
        got = (p.cpu().numpy(), g.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), float(out[0]), float(out[1]))
        ok, _, ratios, why = A.accept(got, sc, k)
        worst = tuple(max(a, b) for a, b in zip(worst, ratios))
        assert ok, (sc, k, why)
        if sc.grad_scale == 0.0:        # norm 0, coefficient 1: the parameters move by weight decay only
            assert got[4] == 0.0 and got[5] == 1.0 and not got[1].any()
            assert np.all((got[0] != args[0]) == (args[4] != 0))
        if sc.max_norm <= 0:
            assert got[5] == 1.0 and np.array_equal(got[1], args[1])
    print(f"\n{sc.name:26s} floors " + " ".join(f"{f:.2e}" for f in floors) + "; kernels / floor "
          + " ".join(f"{r:.2f}" for r in worst))
