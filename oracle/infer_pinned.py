"""The pinned float64 checker of the fp32 inference path, stage by stage (TEST INFRASTRUCTURE, like all of oracle/).

The eval-mode graph of oracle/torch_port.py runs in float64 with every boundary the engine can tap (Engine.tap:
en0..en4, gtcn1, gtcn2, sum4, de0..de4) snapped to the value the HIP kernels stored, and records its own value at each
boundary BEFORE the snap.  Stage k's float64 result is therefore computed from the inputs HIP stage k read: a stage is
charged for its own arithmetic only, never for its predecessors'.

Figures.  Per stage, clip and channel: rms and max of (HIP - checker), divided by that channel's own rms in the
checker (a channel whose checker rms is exactly 0 is compared absolutely, as a class of its own).  The output is
judged the same way per band of 16 bins.  The worst channel of a stage is its figure of merit: a channel 40 dB below
the loudest one counts as much as the loudest.

Yardstick.  No constant: the SAME pinned run in float32 ATen (what the reference executes) against the float64 one
says what "fp32-class" means for that stage at that input.  A channel passes when its rms / max figure is within
MARGINS[stage] x the float32 port's worst-channel figure of the stage (default 1.5x / 2x, the margins of
tests/test_gpu_precision.py) plus that channel's slope allowance.  A margin above the default carries its measured
ratio and its cause beside it (MARGINS); de4, whose tanh has an absolute error on the device, has an absolute allowance
per channel instead (ABS_FLOOR).  The port's worst channel bounds every channel of the stage: a channel is not compared
with the port in the same channel (one channel of one ATen run is too lucky a sample: 4e-10 where a channel is all
negative), so in a stage whose port figure is dominated by one hard channel the others are held less tightly.

The slope allowance.  The kernels' fp32 PReLU is x + (a - 1) * min(x, 0) with a - 1 rounded to fp32 once (kernels.hip
prelu4): the negative branch's slope is off by up to 2^-25 / |a| relatively, coherently over a channel.  That error is
a property of the blob, not of a run, so it is computed, not fitted: a third pinned float64 run on the slopes
fl32(a - 1) + 1 (CONSTS "slope"); a channel's allowance is the same rms / max statistic of that run's deviation from
the clean one.  It is what makes dns3's en0 (slope 0.0131: +2.1e-6 relative) and de3 (slope 0.00122: -9.6e-6) 7x and
20x the port in their mostly-negative quiet channels, and rand's gtcn1 2.3x; with it taken off they are at 0.2, 0.02
and 0.2.  Kept as the kernel has it and allowed for, not fixed: 1e-5 of a channel 50 dB down is far inside the 1e-4
contract, and max(x, 0) + a * min(x, 0) costs one more VALU operation per element on the headline path.

The gtcn2 stage.  k_gtcn_band stores gtcn2(x) + en4 (the decoder's first input); the engine's "gtcn2" tap is that sum
minus en4, subtracted in fp32 on the host (csrc/api.cpp gtcrn_debug_tap), which adds a rounding of the SUM's size that
no kernel made.  The stage is therefore judged on what the kernel stored -- sum4 against (checker gtcn2 + HIP en4) --
in gtcn2's own scale, and the float32 yardstick is formed the same way.  check_sum4 holds the two taps together.

Seeded wrong layers (BUGS).  Each entry changes the float64 graph at ONE stage the way a kernel slip would (the
convention of tests/hybrid_loss_checker.py): the unmodified taps against a checker carrying the bug must fail, and --
everything being pinned -- at that stage and at no other.  The yardstick stays the clean float32-against-clean-float64
figure.
"""
import collections
import re

import numpy as np
import torch
import torch.nn.functional as F

from oracle.torch_port import TorchPort

# engine tap name (Engine.tap) -> TorchPort pin / tap name.  The ONLY place the two namings meet: the engine calls the
# decoder's first input (gtcn2 + en4 as stored) "sum4"; the port counts the decoder's sums from the inside, "sum0".
ENGINE_TO_PORT = collections.OrderedDict(
    [("en0", "en0"), ("en1", "en1"), ("en2", "en2"), ("en3", "en3"), ("en4", "en4"), ("gtcn1", "gtcn1"),
     ("gtcn2", "gtcn2"), ("sum4", "sum0"), ("de0", "de0"), ("de1", "de1"), ("de2", "de2"), ("de3", "de3"),
     ("de4", "de4")])
ENGINE_TAPS = tuple(ENGINE_TO_PORT)
# what the port records and the engine does not hand out: the TCN blocks inside a stack and the decoder's later sums
# (fp64 sums of two pinned tensors; the fp32 rounding of the kernel's own sum belongs to the stage that reads it)
PORT_INTERIOR = tuple(f"tcn{i}" for i in range(8)) + ("sum1", "sum2", "sum3", "sum4")
# the judged boundaries, in graph order; "out" is de4 -> output (inverse ERB + complex mask product)
STAGES = ("en0", "en1", "en2", "en3", "en4", "gtcn1", "gtcn2", "de0", "de1", "de2", "de3", "de4", "out")

DEFAULT_MARGIN = (1.5, 2.0)     # rms, max: the margins of test_forward_is_fp32_class_against_float64
# A stage that needs more than the default: (rms margin, max margin).  Beside each: the worst measured ratio
# (HIP figure - the channel's slope allowance) / float32 port, rms | max, over the cases of
# tests/test_gpu_infer_pinned.py on the MI355X (profiles/infer_stage_pinned.json, "worst_over_cases").  One cause:
#   ORDER  every conv + BatchNorm unit of the kernels is ONE fp32 accumulation chain that STARTS from the folded shift
#          (kernels.hip: `x[i] = Bv` in front of en_convs.1's five tap MFMAs, `mm1(A, bv, Bv)`, `B2 + w0 * ...` in the
#          TCN blocks), so every one of its roundings is made at the size of shift + partial sum; ATen adds the
#          BatchNorm's constants after a blocked sum of the products alone.  simulate_en1_chain reproduces it on the CPU
#          from the blob and the en0 tap, without the device (the report's "en1_chain"): the chain in the kernel's order
#          gives 1.60 x (dns3, white 2x33, channel 10: 1.196e-6; the MI355X measured 1.182e-6 in that channel) and 1.95 x
#          (rand, tilt 2x33, channel 5: 1.141e-6; measured 1.214e-6) the port's worst channel; the same 80 terms in two
#          random orders 1.23 / 1.25 x and 0.94 / 0.62 x, and with the shift added LAST 0.83 x and 0.90 x.  The order of
#          summation alone therefore moves a stage's float32 figure over a range of 0.6 .. 1.95 -- more than a factor 2
#          -- and the stages below get the default margin x 2.  Simulated
#          for en1 only, the stage furthest over; that the other stages' excess has the same cause is supposed from
#          their construction, not shown.  What it is NOT: the BatchNorm fold's own roundings (pack.cpp fold(): weights
#          fl32(w * scale), one constant shift), which CONSTS "fold" puts into the float64 graph -- 0.05 .. 0.9 x the
#          port's figure, incoherent, adding in quadrature (the report's "fold" column).
_ORDER = (2 * DEFAULT_MARGIN[0], 2 * DEFAULT_MARGIN[1])
MARGINS = {
    "en1": _ORDER,          # 2.31 | 2.02  rand tilt 2x2 / dns3 tilt 2x6
    "en2": _ORDER,          # 1.67 | 1.31  dns3 white 1x90 (channel 4 in every dns3 white case)
    "en3": _ORDER,          # 1.43 | 2.18  dns3 tilt 2x2 (the max over 66 elements a channel)
    "gtcn1": _ORDER,        # 2.04 | 2.48  rand tilt 2x2: twelve such units deep
    "gtcn2": _ORDER,        # 1.51 | 2.38  dns3 white 2x16 / rand tilt 2x6: twelve such units deep
    "de0": _ORDER,          # 1.86 | 1.59  dns3 tilt 2x1
    "de1": _ORDER,          # 1.93 | 2.23  dns3 tilt 2x16 / white 2x1
    "de3": _ORDER,          # 0.43 | 2.86  dns3 white 2x17 (max only; the rms is the slope's, see "slope" at CONSTS)
}
# de4 = tanh(...) is computed as 1 - 2 * rcp(exp(2x) + 1) with v_exp_f32 / v_rcp_f32 (kernels.hip fast_tanh): the result
# is 1 minus a number next to 1, so its error is ABSOLUTE -- an ulp of 1.0 whatever |tanh x| is -- where ATen's tanh is
# relative.  Measured on dns3's imaginary-mask channel (rms 8.7e-4): rms 4.1e-8 = 0.70 x 2^-24, max 1.1e-7 = 1.9 x 2^-24
# (74 | 88 x the port's worst channel, 600 x the port in that channel); rand's mask channels are loud and sit at 1.4.
# So a de4 channel also passes within this absolute error of the mask value, over its own rms: (rms, max).
ABS_FLOOR = {"de4": (2.0 ** -24, 4 * 2.0 ** -24)}


def margin(stage):
    return MARGINS.get(stage, DEFAULT_MARGIN)


# ---------------------------------------------------------------------------------------------------- seeded bugs
Bug = collections.namedtuple("Bug", "stage what")
BUGS = collections.OrderedDict([
    ("en2_dw_tap", Bug("en2", "encoder.en_convs.2.depth_conv: tap (kt 1, kf 2) of channel 5 dropped")),
    ("de1_dw_tap", Bug("de1", "decoder.de_convs.1.depth_conv: tap (kt 1, kf 2) of the channel pair 5 -> 9 dropped")),
    ("gtcn1_history_edge", Bug("gtcn1", "gtcn1.blocks.1 (d = 2): tap 0 reads frame t - 2d + 1, not t - 2d, for t < 2d")),
    ("en3_bn_no_eps", Bug("en3", "encoder.en_convs.3.point_bn2: channel 3 folded as 1 / sqrt(var), eps left out")),
    ("en1_prelu_slope", Bug("en1", "encoder.en_convs.1.act: slope off by 2^-10")),
    ("en4_tra_32_bins", Bug("en4", "encoder.en_convs.4.tra: energy averaged over 32 bins, not 33")),
    ("de2_dense_two_planes", Bug("de2", "decoder.de_convs.2: dense 3x3 input as two bf16 planes, the lo plane dropped")),
    ("ierb_band_shift", Bug("out", "erb.ierb_fc: the row of band 20 shifted up by one bin")),
    ("mask_sign", Bug("out", "mask product at bin 40: re*mr + im*mi")),
])
_MASK_BIN = 40          # below bin 65 the mask is de4 itself (no inverse ERB in between)


def _seed_params(p, bug):
    """The slips that are a wrong constant in the packed parameters."""
    if bug == "en2_dw_tap":
        p["encoder.en_convs.2.depth_conv.weight"][5, 0, 1, 2] = 0.0
    elif bug == "de1_dw_tap":
        p["decoder.de_convs.1.depth_conv.weight"][5, 9, 1, 2] = 0.0
    elif bug == "en3_bn_no_eps":
        p["encoder.en_convs.3.point_bn2.running_var"][3] -= 1e-5        # + eps inside batch_norm gives var back
    elif bug == "en1_prelu_slope":
        p["encoder.en_convs.1.act.weight"][0] += 2.0 ** -10
    elif bug == "ierb_band_shift":
        w = p["erb.ierb_fc.weight"]                                     # (192 bins, 64 bands)
        w[:, 20] = torch.roll(w[:, 20].clone(), 1)


def _f32(v):
    return v.to(torch.float32).to(torch.float64)


def _folded_units():
    """(conv, bn, transposed) of every conv + BatchNorm unit the packer folds (csrc/pack.cpp fold() and its callers)."""
    units = [(f"encoder.en_convs.{i}.conv", f"encoder.en_convs.{i}.bn", False) for i in range(2)]
    for pre, dec in [(f"encoder.en_convs.{i}", False) for i in (2, 3, 4)] + \
                    [(f"decoder.de_convs.{i}", True) for i in range(3)]:
        units += [(pre + ".point_conv1", pre + ".point_bn1", dec), (pre + ".depth_conv", pre + ".depth_bn", dec),
                  (pre + ".point_conv2", pre + ".point_bn2", dec)]
    units += [(f"gtcn{g}.blocks.{k}.conv{j}", f"gtcn{g}.blocks.{k}.bn{j}", False)
              for g in (1, 2) for k in range(4) for j in (1, 2, 3)]
    return units + [(f"decoder.de_convs.{i}.conv", f"decoder.de_convs.{i}.bn", True) for i in (3, 4)]


# The constants as the kernels hold them, in the float64 graph: what such a run differs by from the clean one is the
# kernels' DETERMINISTIC error -- computable from the blob alone, no device needed.
#   "slope"  every fp32 PReLU is x + (a - 1) * min(x, 0) with am1 = fl32(a - 1) formed once (kernels.hip prelu4 /
#            slope_arg; the comment at prelu4q states the size): the negative branch's slope is fl32(a - 1) + 1, off by
#            up to 2^-25 absolutely, i.e. 2^-25 / |a| relatively -- 1e-5 for a trained slope of a few 1e-3 -- and
#            COHERENTLY over the whole negative part of every channel the PReLU feeds.
#   "fold"   BatchNorm folded into the conv (pack.cpp fold()): weights fl32(w * gamma / sqrt(var + eps)), the shift
#            one constant fl32((bias - mean) * scale + beta).  Kept for the report (tests/reports/infer_stage_report.py
#            shows that it adds nothing over ATen's own rounding); no bound uses it.
CONSTS = ("slope", "fold")


def _kernel_constants(p, consts):
    if consts == "slope":
        for k in p:
            if re.search(r"act\d?\.weight$", k):
                p[k] = _f32(_f32(p[k]) - 1.0) + 1.0
    elif consts == "fold":
        for conv, bn, transposed in _folded_units():
            s = p[bn + ".weight"] / torch.sqrt(p[bn + ".running_var"] + 1e-5)
            p[conv + ".weight"] = _f32(p[conv + ".weight"] * (s.view(1, -1, 1, 1) if transposed else s.view(-1, 1, 1, 1)))
            shift = _f32((p[conv + ".bias"] - p[bn + ".running_mean"]) * s + p[bn + ".bias"])
            p[conv + ".bias"] = torch.zeros_like(shift)
            p[bn + ".running_mean"], p[bn + ".running_var"] = torch.zeros_like(s), torch.full_like(s, 1.0 - 1e-5)
            p[bn + ".weight"], p[bn + ".bias"] = torch.ones_like(s), shift


class _Checker(TorchPort):
    """The eval-mode port with the pin and, optionally, one entry of BUGS seeded into its graph.  Every layer the bug
    does not name runs TorchPort's own code."""

    def __init__(self, blob, dtype, pin, bug=None, consts=None):
        assert bug is None or bug in BUGS, bug
        assert consts is None or (consts in CONSTS and dtype == torch.float64), consts
        super().__init__(blob, dtype=dtype, pin=pin)
        self.bug = bug
        if bug is not None or consts is not None:
            self.p = {k: v.clone() for k, v in self.p.items()}      # never write through to the caller's blob
            _seed_params(self.p, bug)
            _kernel_constants(self.p, consts)

    def _tra(self, x, pre):
        if self.bug == "en4_tra_32_bins" and pre == "encoder.en_convs.4.tra":
            s = (33.0 / 32.0) ** 0.5            # the gate of x*s is the gate of an energy 33/32 as large
            return super()._tra(x * s, pre) / s
        return super()._tra(x, pre)

    def _tcn(self, x, pre, d):
        if not (self.bug == "gtcn1_history_edge" and pre == "gtcn1.blocks.1"):
            return super()._tcn(x, pre, d)
        p = self.p
        y = F.prelu(self._bn(F.conv2d(x, p[pre + ".conv1.weight"], p[pre + ".conv1.bias"]), pre + ".bn1"),
                    p[pre + ".act1.weight"])
        yp = F.pad(y, [0, 0, 2 * d, 0])
        z = F.conv2d(yp, p[pre + ".conv2.weight"], p[pre + ".conv2.bias"], dilation=(d, 1), groups=16)
        # the slip: for the first 2d frames the oldest tap reads one frame too late (frame 0 instead of history at 2d-1)
        n = min(2 * d, y.shape[2])
        w0 = p[pre + ".conv2.weight"][:, 0, 0, 0].view(1, -1, 1, 1)
        z = torch.cat([z[:, :, :n] + w0 * (yp[:, :, 1:n + 1] - yp[:, :, :n]), z[:, :, n:]], dim=2)
        z = F.prelu(self._bn(z, pre + ".bn2"), p[pre + ".act2.weight"])
        z = self._bn(F.conv2d(z, p[pre + ".conv3.weight"], p[pre + ".conv3.bias"]), pre + ".bn3")
        return F.prelu(z + x, p[pre + ".act3.weight"])

    def _gtconv(self, x, pre, deconv):
        if not (self.bug == "de2_dense_two_planes" and pre == "decoder.de_convs.2"):
            return super()._gtconv(x, pre, deconv)
        assert deconv
        p = self.p
        x1, x2 = x[:, :8], x[:, 8:]
        h = F.conv_transpose2d(x1, p[pre + ".point_conv1.weight"], p[pre + ".point_conv1.bias"])
        h = F.prelu(self._bn(h, pre + ".point_bn1"), p[pre + ".point_act.weight"])
        # the slip: hi + mid of the exact three-plane bf16 split, lo left out
        h32 = h.to(torch.float32)
        hi = h32.to(torch.bfloat16).to(torch.float32)
        h = (hi + (h32 - hi).to(torch.bfloat16).to(torch.float32)).to(h.dtype)
        h = F.conv_transpose2d(h, p[pre + ".depth_conv.weight"], p[pre + ".depth_conv.bias"], padding=(0, 1))
        h = F.prelu(self._bn(h, pre + ".depth_bn"), p[pre + ".depth_act.weight"])
        h = self._bn(F.conv_transpose2d(h, p[pre + ".point_conv2.weight"], p[pre + ".point_conv2.bias"]),
                     pre + ".point_bn2")
        h = self._tra(h, pre + ".tra")[:, :, :x2.shape[2]]
        return torch.stack([h, x2], dim=2).flatten(1, 2)

    def run(self, spec):
        """-> {port tap name: the checker's own value before the pin, float64 numpy} plus "out"."""
        taps = {}
        spec = torch.as_tensor(np.asarray(spec, np.float32))
        out = self.forward(spec, taps).clone()
        if self.bug == "mask_sign":
            m = torch.as_tensor(self.pin["de4"]).to(out.dtype) if self.pin and "de4" in self.pin else taps["de4"]
            re, im = spec[:, _MASK_BIN, :, 0].to(out.dtype), spec[:, _MASK_BIN, :, 1].to(out.dtype)
            out[:, _MASK_BIN, :, 0] = re * m[:, 0, :, _MASK_BIN] + im * m[:, 1, :, _MASK_BIN]
        # (the port also records every conv output in front of a BatchNorm, "<bn>.y": the trainer's points, not ours)
        res = {k: v.numpy().astype(np.float64) for k, v in taps.items() if not k.endswith(".y")}
        res["out"] = out.numpy().astype(np.float64)
        return res


# --------------------------------------------------------------------------------------------------------- inputs
def make_input(kind, B, T, seed=0):
    """(B,257,T,2) float32.  "white": noise x0.3.  "tilt": the speech-like input of test_parity_per_band_and_elementwise,
    -40 dB across the band, loud (x3) in the even clips and quiet (x0.02, over a flat floor of 0.002) in the odd ones."""
    rng = np.random.default_rng(seed)
    if kind == "white":
        return (rng.standard_normal((B, 257, T, 2)) * 0.3).astype(np.float32)
    assert kind == "tilt", kind
    tilt = (10.0 ** (-2.0 * np.arange(257) / 256.0))[:, None, None]
    clips = [rng.standard_normal((257, T, 2)) * tilt * 3.0 if b % 2 == 0 else
             rng.standard_normal((257, T, 2)) * tilt * 0.02 + rng.standard_normal((257, T, 2)) * 0.002 for b in range(B)]
    return np.stack(clips).astype(np.float32)


# ------------------------------------------------------------------------------------------- the HIP side's tensors
def engine_taps(eng, B, T):
    """Every stage tap of every clip of the engine's most recent forward (debug_enable before it): {engine name:
    (B,C,T,F) float32}."""
    return {n: np.stack([eng.tap(n, b, T) for b in range(B)]) for n in ENGINE_TAPS}


def stand_in(blob, spec, dtype=torch.float32, slope_error=0.0):
    """The CPU stand-in for the HIP side: the float32 port's own UNPINNED taps under the engine's names, and its
    output.  sum4 is formed as the kernel stores it, fp32(gtcn2 + en4).  slope_error (float64 only): every PReLU slope
    moved by that multiple of the kernels' rounding error fl32(a - 1) + 1 - a (1.0: the slopes the kernels use)."""
    taps = {}
    port = TorchPort(blob, dtype=dtype)
    if slope_error:
        assert dtype == torch.float64
        k = _Checker(blob, torch.float64, None, consts="slope")
        port.p = {n: v + slope_error * (k.p[n] - v) for n, v in port.p.items()}
    out = port.forward(torch.as_tensor(np.asarray(spec, np.float32)), taps)
    got = {n: taps[ENGINE_TO_PORT[n]].numpy().astype(np.float32) for n in ENGINE_TAPS}
    return got, out.numpy().astype(np.float32)


def check_sum4(taps):
    """The engine's sum4 (the decoder's first input, as stored) is fp32(gtcn2 + en4) of its own taps, bit for bit."""
    want = taps["gtcn2"].astype(np.float32) + taps["en4"].astype(np.float32)
    same = want.view(np.uint32) == np.ascontiguousarray(taps["sum4"], np.float32).view(np.uint32)
    assert same.all(), (f"sum4 != fp32(gtcn2 + en4) at {int((~same).sum())} of {same.size} elements, first at "
                        f"{tuple(int(i) for i in np.argwhere(~same)[0])}")


def _pin(taps):
    missing = [n for n in ENGINE_TAPS if n not in taps]
    assert not missing, f"taps missing: {missing}"
    return {ENGINE_TO_PORT[n]: torch.from_numpy(np.ascontiguousarray(taps[n], np.float32)) for n in ENGINE_TAPS}


def pinned_run(blob, spec, taps, dtype=torch.float64, bug=None, consts=None):
    """The pinned graph in `dtype`: its own value at every boundary before the snap (port names) and "out".  consts:
    one of CONSTS -- the float64 graph on the constants as the kernels hold them (_kernel_constants)."""
    return _Checker(blob, dtype, _pin(taps), bug, consts).run(spec)


# ------------------------------------------------------------------------------------------------------- figures
def _groups(stage, a):
    """(B, groups, elements...) view of a stage tensor: channels, or bands of 16 bins for the output."""
    if stage != "out":
        return [a[:, c] for c in range(a.shape[1])]
    return [a[:, lo:lo + 16] for lo in range(0, a.shape[1], 16)]


def _stage_pair(stage, got, chk, hip):
    """(value under test, checker value, checker tensor whose channel rms normalises) for one stage."""
    if stage == "gtcn2":        # judged on the stored sum, in gtcn2's own scale (module docstring)
        e4 = hip["en4"].astype(np.float64)
        return got["sum4"].astype(np.float64), chk["gtcn2"] + e4, chk["gtcn2"]
    c = chk[stage if stage == "out" else ENGINE_TO_PORT[stage]]
    return got[stage].astype(np.float64), c, c


def stage_figures(stage, got, chk, hip):
    """Per (clip, group): rms and max of the error over the group's checker rms.  -> (rms (B,G), max (B,G), zero (B,G),
    den (B,G)): `zero` marks the groups whose checker rms is exactly 0, whose two figures are absolute (den = 1)."""
    a, c, ref = _stage_pair(stage, got, chk, hip)
    assert a.shape == c.shape, (stage, a.shape, c.shape)
    B = a.shape[0]
    ga, gc, gr = _groups(stage, a), _groups(stage, c), _groups(stage, ref)
    rms, mx, zero, dens = (np.zeros((B, len(ga))) for _ in range(4))
    for g in range(len(ga)):
        err = (ga[g] - gc[g]).reshape(B, -1)
        den = np.sqrt((gr[g].reshape(B, -1) ** 2).mean(axis=1))
        z = den == 0.0
        den = np.where(z, 1.0, den)
        rms[:, g], mx[:, g], zero[:, g] = np.sqrt((err ** 2).mean(axis=1)) / den, np.abs(err).max(axis=1) / den, z
        dens[:, g] = den
    return rms, mx, zero.astype(bool), dens


def _worst(fig, mask, bound=None):
    """(value, clip, group) of the largest figure among the masked groups -- with `bound` (B,G): of the figure furthest
    over its own bound; (0, -1, -1) if there is none."""
    if not mask.any():
        return 0.0, -1, -1
    f = np.where(mask, fig if bound is None else fig / np.maximum(bound, 1e-300), -1.0)
    b, g = np.unravel_index(int(np.argmax(f)), f.shape)
    return float(fig[b, g]), int(b), int(g)


# hip: the figure of the channel furthest over its own bound, at (clip, group), `bound` and `allow` (the slope allowance
# inside the bound) being that channel's; worst: the stage's largest HIP figure whatever its bound; port: the float32
# port's largest
Row = collections.namedtuple("Row", "stage stat cls hip clip group port bound ok worst allow")


def _as_got(run, taps):
    """A pinned run's own values under the engine's names, sum4 as the kernel forms it: ITS gtcn2 plus the en4 both read."""
    got = {n: run[ENGINE_TO_PORT[n]] for n in ENGINE_TAPS}
    got["sum4"] = run["gtcn2"] + taps["en4"].astype(np.float64)
    got["out"] = run["out"]
    return got


def yardstick(blob, spec, taps, clean=None):
    """What the bounds are made of, both against the clean float64 run: {"port": the float32 port's pinned run, "slope":
    the float64 run on the kernels' rounded slope-minus-one (CONSTS)}, each {stage: stage_figures}.  Bug runs reuse it."""
    clean = clean if clean is not None else pinned_run(blob, spec, taps)
    p32 = _as_got(pinned_run(blob, spec, taps, dtype=torch.float32), taps)
    p32["sum4"] = (p32["gtcn2"].astype(np.float32) + taps["en4"].astype(np.float32)).astype(np.float64)   # an fp32 sum
    slope = _as_got(pinned_run(blob, spec, taps, consts="slope"), taps)
    return {"port": {s: stage_figures(s, p32, clean, taps) for s in STAGES},
            "slope": {s: stage_figures(s, slope, clean, taps) for s in STAGES}}


def simulate_en1_chain(blob, en0, order="kernel", seed=0):
    """en_convs.1 on the CPU the way k_front accumulates it (MARGINS, ORDER): BatchNorm folded as pack.cpp folds it, one
    fp32 FMA chain per output over the 80 terms, tap major, started from the shift, then prelu4.  order "kernel";
    "random": the same chain over a random permutation of the terms; "shift_last": started from 0, the shift added last.
    en0: (B,16,T,65) float32 -> (B,16,T,33) float32.  For the report, which sets its figure beside the device's."""
    p = {k: v.double().numpy() for k, v in _Checker(blob, torch.float64, None).p.items()}
    pre = "encoder.en_convs.1"
    s = p[pre + ".bn.weight"] / np.sqrt(p[pre + ".bn.running_var"] + 1e-5)
    w = (p[pre + ".conv.weight"] * s[:, None, None, None]).astype(np.float32).astype(np.float64)
    sh = ((p[pre + ".conv.bias"] - p[pre + ".bn.running_mean"]) * s + p[pre + ".bn.bias"]).astype(np.float32)
    am1 = np.float64(np.float32(np.float32(p[pre + ".act.weight"][0]) - np.float32(1.0)))
    x = np.pad(np.asarray(en0, np.float32), [(0, 0), (0, 0), (0, 0), (2, 2)]).astype(np.float64)
    B, _, T, W = x.shape
    F1 = (W - 5) // 2 + 1
    terms = [(c, k) for k in range(5) for c in range(16)]
    if order == "random":
        terms = [terms[i] for i in np.random.default_rng(seed).permutation(len(terms))]
    acc = np.zeros((B, 16, T, F1), np.float32)
    if order != "shift_last":
        acc += sh[None, :, None, None]
    for c, k in terms:      # the product of two fp32 numbers is exact in float64: one rounding per term, as an FMA
        acc = (acc.astype(np.float64) + w[None, :, c, 0, k, None, None] * x[:, None, c, :, k:k + 2 * F1 - 1:2]).astype(np.float32)
    if order == "shift_last":
        acc = acc + sh[None, :, None, None]
    return (acc.astype(np.float64) + am1 * np.minimum(acc, 0).astype(np.float64)).astype(np.float32)


def measure(blob, spec, taps, out, bug=None, yard=None):
    """The table: one Row per stage, statistic (rms / max) and class (rel: normalised by the channel's rms; abs: channels
    whose checker rms is exactly 0).  A channel's bound is margin x the float32 port's worst channel of the stage plus that
    channel's own slope allowance (the same statistic of the "slope" run's deviation, module docstring); where the stage
    has an absolute allowance (ABS_FLOOR) the bound is at least that allowance over the channel's rms.  The row names the
    channel furthest over its own bound (band of 16 bins for "out")."""
    hip = dict(taps)
    hip["out"] = np.asarray(out)
    chk = pinned_run(blob, spec, taps, bug=bug)
    yard = yard if yard is not None else yardstick(blob, spec, taps, chk if bug is None else None)
    rows = []
    for s in STAGES:
        h, p, a = stage_figures(s, hip, chk, taps), yard["port"][s], yard["slope"][s]
        for cls, hm, pm in (("rel", ~h[2], ~p[2]), ("abs", h[2], p[2])):
            if not hm.any():
                continue
            for k, stat in enumerate(("rms", "max")):
                pv = _worst(p[k], pm)[0]
                allow = a[k] * a[3] / h[3]          # in this run's scale (a seeded bug moves a channel's rms a little)
                bounds = margin(s)[k] * pv + allow
                if s in ABS_FLOOR and cls == "rel":
                    bounds = np.maximum(bounds, ABS_FLOOR[s][k] / h[3])
                hv, b, g = _worst(h[k], hm, bounds)
                bound = float(bounds[b, g])
                rows.append(Row(s, stat, cls, hv, b, g, pv, bound, bool(hv <= bound), _worst(h[k], hm)[0],
                                float(allow[b, g])))
    return rows


def failing_stages(rows):
    return sorted({r.stage for r in rows if not r.ok}, key=STAGES.index)


def distance(rows, stage):
    """Largest failing figure / bound at a stage (how far a seeded bug is rejected); inf over a zero bound."""
    return max((r.hip / r.bound if r.bound > 0 else float("inf")) for r in rows if r.stage == stage)


def fmt(r):
    what = "band" if r.stage == "out" else "channel"
    return (f"{r.stage}: clip {r.clip} {what} {r.group}: {r.stat} error / {what} rms {r.hip:.3e} "
            f"({'absolute, ' if r.cls == 'abs' else ''}float32 port {r.port:.3e}, slope allowance {r.allow:.3e}, "
            f"bound {r.bound:.3e}; worst {what} of the stage {r.worst:.3e})")


def _ratio(a, b):
    return a / b if b > 0 else (0.0 if a <= 0 else float("inf"))


def ratios(rows):
    """{stage: ((rms, max) of worst HIP channel / the port's worst, (rms, max) of the same with the slope allowance of the
    channel furthest over its bound taken off first: what the margin has to cover)}."""
    raw, net = {}, {}
    for r in rows:
        k = r.stage, r.stat
        raw[k] = max(raw.get(k, 0.0), _ratio(r.worst, r.port))
        net[k] = max(net.get(k, 0.0), _ratio(r.hip - r.allow, r.port))
    return {s: ((raw[s, "rms"], raw[s, "max"]), (net[s, "rms"], net[s, "max"])) for s in STAGES}


def summary(rows):
    """One line: per stage the worst HIP / float32-port ratio of the rms and of the max figure, and after "-" the same
    with the slope allowance taken off."""
    return "HIP / float32 port, rms|max - net of the slope allowance: " + " ".join(
        f"{s} {a[0]:.2f}|{a[1]:.2f}-{b[0]:.2f}|{b[1]:.2f}" for s, (a, b) in ratios(rows).items())


def assert_pinned_forward(blob, spec, taps, out, what="", verbose=False):
    """Raises with stage, clip, channel and both figures of every stage figure outside margin x the float32 port's; and if
    the engine's sum4 is not fp32(gtcn2 + en4) of its own taps.  Returns the table (verbose: prints its summary first)."""
    rows = measure(blob, spec, taps, out)
    if verbose:
        print(f"[{what}] {summary(rows)}")
    check_sum4(taps)
    bad = [r for r in rows if not r.ok]
    assert not bad, f"{what}: " + "; ".join(fmt(r) for r in bad)
    return rows
