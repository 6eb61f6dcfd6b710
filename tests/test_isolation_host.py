"""The influence cone of one non-finite input element, pinned on the CPU references: the float64 PyTorch port
(oracle/torch_port.py) and the C oracle (oracle/oracle.py, used as tests/test_oracle_golden.py uses it).  tests/test_gpu_isolation.py asserts these sets on the kernels;
the numbers come from here and from isolation_checker's derivation, never from a GPU run."""
import numpy as np
import pytest

import isolation_checker as IC
from conftest import load_params

torch = pytest.importorskip("torch")

B, T = 2, 120
HOPS = 110


@pytest.fixture(scope="module")
def spec():
    rng = np.random.default_rng(85)
    return (rng.standard_normal((B, IC.NBINS, T, 2)) * 0.3).astype(np.float32)


@pytest.fixture(scope="module")
def wave():
    rng = np.random.default_rng(87)
    return (rng.standard_normal((B, 256 * HOPS)) * 0.1).astype(np.float32)


class _Port64:
    name = "torch_port_f64"

    def __init__(self, tag):
        from oracle.torch_port import TorchPort
        self.m = TorchPort(load_params(tag), dtype=torch.float64)
        self.win = torch.hann_window(512).pow(0.5)

    def forward(self, s):
        return self.m.forward(s).numpy()

    def enhance(self, w):
        return self.m.enhance(w, self.win).numpy()


class _COracle:
    name = "c_oracle_f32"

    def __init__(self, tag):
        from oracle import oracle as O
        self.m = O.Oracle(load_params(tag))

    def forward(self, s):
        return self.m.forward(s)

    def enhance(self, w):
        return self.m.enhance(w)


_CACHE = {}


def _model(kind, tag):
    if (kind, tag) not in _CACHE:
        _CACHE[kind, tag] = _COracle(tag) if kind == "c" else _Port64(tag)
    return _CACHE[kind, tag]


_CLEAN = {}


def _clean(kind, tag, what, x):
    """The clean run of a model, computed once and never modified."""
    key = (kind, tag, what)
    if key not in _CLEAN:
        m = _model(kind, tag)
        _CLEAN[key] = m.forward(x) if what == "spec" else m.enhance(x)
        _CLEAN[key].setflags(write=False)
    return _CLEAN[key]


def test_cone_is_derived_from_the_halos():
    assert IC.CONE == 1 + 2 * IC.HALO_BLOCKS + 2 * IC.HALO_GTCN == 85
    assert IC.cone_frames(7, 120) == set(range(7, 92))
    assert IC.cone_frames(117, 120) == {117, 118, 119}
    assert IC.cone_blocks(9, 110) == set(range(8, 95)) and len(IC.cone_blocks(9, 110)) == 87
    assert IC.cone_blocks(0, 110) == set(range(0, 86))
    assert IC.cone_blocks(109, 110) == {108, 109}


def test_halos_are_the_kernels():
    """The two constants the cone is derived from are the ones kernels.hip's time spans recompute."""
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "gtcrn_micro_amd", "csrc", "kernels.hip")).read()
    for name, val in (("HALO_BLOCKS", IC.HALO_BLOCKS), ("HALO_GTCN", IC.HALO_GTCN)):
        m = re.search(rf"\b{name}\s*=\s*(\d+)", src)
        assert m and int(m.group(1)) == val, name


def test_helpers():
    a = np.array([1.0, np.nan, np.inf, 0.0], np.float32)
    b = a.copy()
    assert IC.same_bits(a, b) and IC.same_bits_or_both_nonfinite(a, b)
    b[3] = -0.0
    assert not IC.same_bits(a, b) and not IC.same_bits_or_both_nonfinite(a, b)
    b[3] = 0.0
    b[1] = -np.inf
    assert not IC.same_bits(a, b) and IC.same_bits_or_both_nonfinite(a, b)
    b[0] = np.nan
    assert not IC.same_bits_or_both_nonfinite(a, b)
    x = np.zeros((3, 5, 2), np.float32)
    x[:, 1] = np.nan
    x[0, 3, 1] = np.inf
    assert IC.nonfinite_frames(x, axis=1) == {1: True, 3: False}
    w = np.zeros(600, np.float32)
    w[256:512] = np.nan
    w[599] = np.nan
    assert IC.nonfinite_frames(w, block=256) == {1: True, 2: False}
    assert IC.resample_range(3001, 1, 3, 96, 2000) == (969, 1032)
    assert IC.resample_range(0, 3, 1, 96, 18000) == (0, 96)


def test_no_designed_resampling_tap_is_zero():
    """What makes the resampler's non-finite range exact (include/gtcrn_micro_hip.h): for all 14 supported pairs no tap the
    kernels use is zero, in float32 as in the float64 definition -- only the phase tables' padding is, and it reads no
    sample."""
    import resample_checker as RC
    from gtcrn_micro_amd._lib import resample_taps
    assert len(RC.PAIRS) == 14
    for fs_in, fs_out in RC.PAIRS:
        up, down, half, h64 = RC.design(fs_in, fs_out)
        u, d, h = resample_taps(fs_in, fs_out)
        assert (u, d, len(h)) == (up, down, 2 * half + 1), (fs_in, fs_out)
        assert h.dtype == np.float32 and (h != 0).all() and (h64 != 0).all(), (fs_in, fs_out)


SPEC_POISONS = ["nan_bin", "nan_frame", "inf_frame", "huge_frame"]


def _poison_spec(spec, how, t0):
    s = spec.copy()
    if how == "nan_bin":
        s[0, 200, t0, 0] = IC.QNAN
    else:
        s[0, :, t0, :] = {"nan_frame": IC.QNAN, "inf_frame": IC.PINF, "huge_frame": IC.HUGE}[how]
    return s


@pytest.mark.parametrize("t0", [7, T - 3])
@pytest.mark.parametrize("how", SPEC_POISONS)
@pytest.mark.parametrize("tag", ["dns3", "rand"])
@pytest.mark.parametrize("kind", ["f64", "c"])
def test_spectrum_cone(spec, kind, tag, how, t0):
    """Poison in utterance 0, frame t0: utterance 1 and the frames outside t0 .. t0 + 84 keep their bits; NaN and Inf make
    every bin of every frame of the cone non-finite; 1e30 stays finite in float64 and changes the cone only."""
    clean = _clean(kind, tag, "spec", spec)
    got = _model(kind, tag).forward(_poison_spec(spec, how, t0))
    cone = IC.cone_frames(t0, T)
    keep = [t for t in range(T) if t not in cone]
    assert IC.same_bits(got[1], clean[1])
    assert IC.same_bits(got[0][:, keep], clean[0][:, keep])
    bad = IC.nonfinite_frames(got[0], axis=1)
    if how == "huge_frame":
        if kind == "f64":
            assert not bad
        differs = {t for t in range(T) if not IC.same_bits(got[0][:, t], clean[0][:, t])}
        assert differs <= cone and t0 in differs
    else:
        assert bad == {t: True for t in cone}


@pytest.mark.parametrize("sample,blocks", [(256 * 9 + 100, range(8, 95)), (5, range(0, 86)), (256 * 109 + 100, range(108, 110)),
                                           (256 * 50 + 128, range(49, 110))])
@pytest.mark.parametrize("tag", ["dns3", "rand"])
@pytest.mark.parametrize("kind", ["f64", "c"])
def test_wave_cone(wave, kind, tag, sample, blocks):
    """A NaN sample inside hop h: output blocks h - 1 .. h + 85 (clipped to the clip) are non-finite in every sample, every
    other block and the neighbour clip keep their bits."""
    clean = _clean(kind, tag, "wave", wave)
    w = wave.copy()
    w[0, sample] = IC.QNAN
    got = _model(kind, tag).enhance(w)
    assert set(blocks) == IC.cone_blocks(sample // 256, HOPS)
    assert IC.same_bits(got[1], clean[1])
    assert IC.nonfinite_frames(got[0], block=256) == {b: True for b in blocks}
    keep = np.ones(got.shape[1], bool)
    keep[256 * blocks[0]:256 * (blocks[-1] + 1)] = False
    assert IC.same_bits(got[0][keep], clean[0][keep])
