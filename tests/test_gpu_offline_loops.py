"""The offline kernels' loops carry their indices instead of rebuilding them: k_gtcn_band steps one row counter per chunk
and keeps one per-lane offset (clamped in the final, partial chunk), k_front steps (utterance, frame) by a constant stride
with one carry.  The shapes below are the smallest at which a carried or hoisted index can be wrong.  Needs a real MI355X:
run with `-m gpu`.  Tolerance against the oracle: conftest.check_parity, what tests/test_gpu_parity.py holds the whole
path to; everything else is bit equality."""
import numpy as np
import pytest

from conftest import check_parity, load_params

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# T = 3, 18, 34 frames: less than one 16-frame chunk; one chunk and a two-frame partial one; two chunks and two frames
# (there the D = 8 ring of the GTCN has wrapped and the carried offsets have stepped twice)
LENGTHS = (512, 4352, 8448)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as graft
    graft.build()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def eng(dev):
    from gtcrn_micro_amd import Engine
    return Engine(load_params("dns3"), 0)


@pytest.fixture(scope="module")
def win(dev):
    import gtcrn_micro_amd as G
    return torch.from_numpy(G.make_window(0)).cuda()


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O.Oracle(load_params("dns3"))


def clips(B, L):
    return (np.random.default_rng(1000 * B + L).standard_normal((B, L)) * 0.1).astype(np.float32)


@pytest.fixture(scope="module")
def batch3(eng, win):
    """L -> (input, B = 3 result), computed once and read by several tests"""
    out = {}
    for L in LENGTHS:
        x = torch.from_numpy(clips(3, L)).cuda()
        out[L] = (x, eng.forward_wave(x, win))
    return out


@pytest.mark.parametrize("L", LENGTHS)
def test_chunk_boundaries_vs_oracle(batch3, oracle, L):
    x, y = batch3[L]
    assert tuple(y.shape) == (3, 256 * (L // 256))
    check_parity(y.cpu().numpy(), oracle.enhance(x.cpu().numpy()), f"B=3 L={L}")


@pytest.mark.parametrize("L", LENGTHS)
def test_batch_invariance(eng, win, batch3, L):
    """a B = 1 call takes the time-span kernels: each clip of the batch equals its own call, bit for bit"""
    x, y = batch3[L]
    for b in range(3):
        assert torch.equal(eng.forward_wave(x[b:b + 1].clone(), win)[0], y[b]), (L, b)


def test_variable_lengths_equal_fixed_length_calls(eng, win):
    """k_front steps (utterance, frame) across utterance boundaries and skips the frames past a clip's end"""
    lens = [512, 4352, 8448, 8448 - 256]
    x = clips(4, max(lens))
    xg = torch.from_numpy(x).cuda()
    y = eng.forward_wave_var(xg, lens, win)
    for b, n in enumerate(lens):
        want = eng.forward_wave(xg[b:b + 1, :n].contiguous(), win)[0]
        assert tuple(want.shape) == (256 * (n // 256),)
        assert torch.equal(y[b, :want.numel()], want), (b, n)


@pytest.mark.parametrize("B,L", [(40, 512), (1, 64000)])
def test_front_frame_loop_vs_oracle(eng, win, oracle, B, L):
    """B * T = 120 frames: fewer than one stride of the persistent front-end grid, every wave has at most one frame;
    B = 1, L = 64000: many strides land on one utterance"""
    x = clips(B, L)
    y = eng.forward_wave(torch.from_numpy(x).cuda(), win)
    check_parity(y.cpu().numpy(), oracle.enhance(x), f"B={B} L={L}")


def test_streaming_equals_offline_bit_for_bit(eng):
    """the streaming forms (shared helpers) against the offline kernels at T = 18"""
    spec = torch.from_numpy((np.random.default_rng(18).standard_normal((2, 257, 18, 2)) * 0.3).astype(np.float32)).cuda()
    st = eng.new_state(2)
    stepped = torch.cat([eng.stream_step(st, spec[:, :, t:t + 1]) for t in range(18)], 2)
    assert torch.equal(stepped, eng.forward_spec(spec))
