"""Checker of the int8-weight / fp16-activation variant (BASELINE configs[4]) -- TEST INFRASTRUCTURE ONLY.

PARITY UNPINNED: the reference ships no quantised model, calibration data or TensorFlow, so there is
nothing of the reference's to compare numbers with.  This file restates, as plain PyTorch-CPU ops, the contract
written in include/gtcrn_micro_hip.h (gtcrn_forward_spec_quant) from the reference's own pieces:

  * graph: GTCRNMicro.forward in eval mode (models/gtcrn_micro.py:506-532), BatchNorm folded into the preceding
    conv (what the exported graph holds), PReLU as the ReLU composite of `-rtpo PReLU` (same function);
  * weights: symmetric int8 per OUTPUT channel (onnx2tf `-oiqt -qt per-channel`, scripts/onnx2tf.sh:50-64),
    scale = max|w| / 127, consumed as fp16(q * scale);
  * activations: rounded to fp16 (RNE) where a layer produces them; sums and products in fp32;
  * optional int8 boundary: x_q = clip(round(x / (scale/255)), -128, 127) (tflite_infer.py:79-92, zero point 0;
    scale = 19.944473, streaming/tflite/calib_scale.txt; utils/calibration_data.py:97-106).

The HIP kernels accumulate in a different order than ATen, so values differ by fp32 rounding BEFORE each fp16
rounding: a fraction of the elements lands on the neighbouring fp16 value (2^-11 relative).  Tests state the tolerance.

Summation order.  QuantPort(blob, acc="f64") forms every conv / linear / energy sum in float64 from the same
fp16-valued operands and rounds it once to float32 and then to fp16 at exactly the places where acc="f32" (ATen's
float32 sums, the default) rounds to fp16.  split=True forms every conv / linear sum as two float32 sums over the two
halves of its reduction, added: a third order.  The distance between two of them is the flip-noise floor of the contract
(tests/quant_cases.py); the kernels' MFMA k-order is one more draw of the same noise.

Transcendentals.  fn="aten" (default) calls ATen's sqrt / sigmoid / tanh in self.dt.  fn="kernel" evaluates, in float32,
the forms the header names for the kernels: sigmoid(z) = 1 / (1 + exp(-z)), tanh(x) = 1 - 2 / (exp(2x) + 1) (sqrt is the
float32 square root either way).  The second tanh form cancels for small |x| (absolute error ~1e-7, a large relative
error of a small mask value that is about to be rounded to fp16): one more stand-in for the floors of the stages that
hold such a function (tests/quant_cases.py: TRANSCENDENTAL_STAGES).

Stage taps and pins.  forward(..., pins=, taps=) works at the 13 boundaries STAGES: en0..en4 (encoder outputs), gtcn1
(first stack), sum4 (h16(gtcn2(x) + en4), the decoder's first input -- what the kernels store), de0..de2 (block
outputs BEFORE the skip sum, which belongs to the next stage), de3, de4 (the tanh mask, (B,2,T,129)) and out (the
result).  `taps` (a dict) receives the checker's own float32 value at each boundary, (B,C,T,F); `pins` (a dict, any
subset) replaces it with the given one before anything downstream reads it -- the skip connections included.  Pinned to
a device's taps, every stage is evaluated from the device's own stage inputs: differences no longer avalanche past one
stage (tests/quant_cases.py: accept_stages).  With neither argument nothing changes, bit for bit.

Mutants.  QuantPort(..., mutate=name) seeds ONE bug in ONE place (MUTANTS below: name -> (stage it is seeded in, what
it is)): what a checker of this variant has to reject.  They exist for tests/test_quant_checker.py only.
"""
import numpy as np
import torch
import torch.nn.functional as F

from .torch_port import blob_to_dict

CALIB_SCALE = 19.944473266601562          # streaming/tflite/calib_scale.txt:1


def h16(x):
    """Round to binary16 (through float32 when x is float64: once to float32, then to fp16); dtype is kept."""
    return x.float().half().to(x.dtype)


def quant_step(scale):
    """The quantiser step the library uses: the float32 quotient scale / 255 (include/gtcrn_micro_hip.h)."""
    return np.float32(np.float32(scale) / np.float32(255.0))


def int8_boundary(x, scale, lo=-128, ties_away=False):
    """float32 in, float32 out: clip(rint(x / step), -128, 127) * step, ties to even."""
    x = x.float()
    step = quant_step(scale)
    r = x / step
    r = torch.sign(r) * torch.floor(r.abs() + 0.5) if ties_away else torch.round(r)
    return torch.clamp(r, lo, 127) * step


def quant_per_out_channel(w, out_dim=0, per_tensor=False):
    """w -> fp16(int8 * scale), one scale per index of `out_dim` (per_tensor: one for all -- a seeded bug)."""
    w = w.double()
    dims = list(range(w.dim())) if per_tensor else [d for d in range(w.dim()) if d != out_dim]
    mx = w.abs().amax(dim=dims, keepdim=True)
    scale = (mx / 127.0).float().double()
    q = torch.where(scale > 0, torch.clamp(torch.round(w / torch.where(scale > 0, scale, torch.ones_like(scale))),
                                           -127, 127), torch.zeros_like(w))
    return h16((q * scale).float())


STAGES = ("en0", "en1", "en2", "en3", "en4", "gtcn1", "sum4", "de0", "de1", "de2", "de3", "de4", "out")

# name -> (the stage the bug is seeded in, the one place).  The two boundary mutants change the quantised spectrogram,
# which the first stage AND the mask product of the last one read (BOUNDARY_MUTANTS: also seen in "out").
MUTANTS = {
    "drop_tap": ("en3", "encoder.en_convs.3.depth_conv: tap (current frame, centre bin) of channel 0 set to 0"),
    "drop_tcn_tap": ("sum4", "gtcn2.blocks.3.conv2 (d = 8): the oldest tap (16 frames back) set to 0"),
    "no_round": ("de1", "decoder.de_convs.1.point_conv2: its fp16 rounding skipped"),
    "per_tensor_scale": ("en2", "encoder.en_convs.2.point_conv2: one weight scale for the tensor, not one per output channel"),
    "clamp127": ("en0", "input boundary clamped to -127 .. 127"),
    "ties_away": ("en0", "input and output boundary round half away from zero"),
    "tra_hist": ("en4", "encoder.en_convs.4.tra: one frame of energy history instead of two"),
    "skip_unrounded": ("de1", "decoder.de_convs.1: its skip sum x + skips[3] left unrounded"),
    "stale_hist_16": ("en2", "encoder.en_convs.2.depth_conv: the two history rows zero at every frame = 0 mod 16"),
    # one missed rounding each: invisible at the output once the flip noise has saturated, plain under pins
    "mag_unrounded": ("en0", "the magnitude sqrt(re^2 + im^2 + 1e-12): its fp16 rounding skipped"),
    "en1_unrounded": ("en1", "encoder.en_convs.1: the fp16 rounding of its PReLU output skipped"),
    "tcn1_act2_unrounded": ("gtcn1", "gtcn1.blocks.2.act2: its fp16 rounding skipped"),
    "tcn2_act3_unrounded": ("sum4", "gtcn2.blocks.0.act3: its fp16 rounding skipped"),
    "gate_unrounded": ("en3", "encoder.en_convs.3.tra: the sigmoid gate left unrounded"),
    "de3_unrounded": ("de3", "decoder.de_convs.3: the fp16 rounding of its PReLU output skipped"),
    "ierb_unrounded": ("out", "the inverse-ERB sum of the mask: its fp16 rounding skipped"),
}
BOUNDARY_MUTANTS = ("clamp127", "ties_away")


class QuantPort:
    def __init__(self, blob, acc="f32", mutate=None, split=False, fn="aten"):
        assert acc in ("f32", "f64") and (mutate is None or mutate in MUTANTS) and not (split and acc != "f32")
        assert fn in ("aten", "kernel") and not (fn == "kernel" and acc != "f32")
        self.dt = torch.float64 if acc == "f64" else torch.float32
        self.mutate, self.split, self.fn = mutate, split, fn
        p = {k: v.double() for k, v in blob_to_dict(blob).items()}
        self.p = p
        self.w, self.b = {}, {}

        def fold(conv, bn, transposed):
            s = p[bn + ".weight"] / torch.sqrt(p[bn + ".running_var"] + 1e-5)
            w = p[conv + ".weight"]
            w = w * (s.view(1, -1, 1, 1) if transposed else s.view(-1, 1, 1, 1))
            bias = p.get(conv + ".bias")
            bias = torch.zeros_like(s) if bias is None else bias
            per_tensor = mutate == "per_tensor_scale" and conv == "encoder.en_convs.2.point_conv2"
            self.w[conv] = quant_per_out_channel(w.float(), 1 if transposed else 0, per_tensor)
            self.b[conv] = ((bias - p[bn + ".running_mean"]) * s + p[bn + ".bias"]).float()
        for i in range(2):
            fold(f"encoder.en_convs.{i}.conv", f"encoder.en_convs.{i}.bn", False)
        for pre, dec in [(f"encoder.en_convs.{i}", False) for i in (2, 3, 4)] + \
                        [(f"decoder.de_convs.{i}", True) for i in range(3)]:
            fold(pre + ".point_conv1", pre + ".point_bn1", dec)
            fold(pre + ".depth_conv", pre + ".depth_bn", dec)
            fold(pre + ".point_conv2", pre + ".point_bn2", dec)
            self.w[pre + ".tra.depth_conv"] = quant_per_out_channel(p[pre + ".tra.depth_conv.weight"].float())
            self.w[pre + ".tra.point_conv"] = quant_per_out_channel(p[pre + ".tra.point_conv.weight"].float())
        for g in (1, 2):
            for k in range(4):
                pre = f"gtcn{g}.blocks.{k}"
                for j in (1, 2, 3):
                    fold(f"{pre}.conv{j}", f"{pre}.bn{j}", False)
        fold("decoder.de_convs.3.conv", "decoder.de_convs.3.bn", True)
        fold("decoder.de_convs.4.conv", "decoder.de_convs.4.bn", True)
        self.w["erb"] = quant_per_out_channel(p["erb.erb_fc.weight"].float())
        self.w["ierb"] = quant_per_out_channel(p["erb.ierb_fc.weight"].float())
        self.w["sfe"] = quant_per_out_channel(p["sfe.depth_conv.weight"].float())
        if mutate == "drop_tap":
            self.w["encoder.en_convs.3.depth_conv"][0, 0, 2, 1] = 0.0
        if mutate == "drop_tcn_tap":
            self.w["gtcn2.blocks.3.conv2"][:, :, 0, :] = 0.0
        if mutate == "tra_hist":
            self.w["encoder.en_convs.4.tra.depth_conv"][:, :, 0] = 0.0
        self.w = {k: v.to(self.dt) for k, v in self.w.items()}
        self.b = {k: v.to(self.dt) for k, v in self.b.items()}
        self.f = {k: v.float().to(self.dt) for k, v in p.items()}

    def _sum(self, fn, x, w, b=None, **kw):
        """One conv / linear: its sums in self.dt; split: over the two halves of the weight tensor's elements (a
        zeroed weight adds an exact 0, so each call IS the float32 sum of its half), added, then the bias."""
        if not self.split:
            return fn(x, w, b, **kw)
        half = (torch.arange(w.numel()).view(w.shape) % 2 == 0) if w.numel() > 1 else torch.ones_like(w, dtype=torch.bool)
        y = fn(x, torch.where(half, w, torch.zeros_like(w)), None, **kw) + \
            fn(x, torch.where(half, torch.zeros_like(w), w), None, **kw)
        if b is not None:
            y = y + b.view([1, -1] + [1] * (y.dim() - 2)) if fn is not F.linear else y + b
        return y

    def _rnd(self, x, site):
        """h16, unless the mutant is the missed rounding at `site`."""
        return x if site is not None and self.mutate == site else h16(x)

    def _sigmoid(self, z):
        return torch.reciprocal(1.0 + torch.exp(-z)) if self.fn == "kernel" else torch.sigmoid(z)

    def _tanh(self, x):
        return 1.0 - 2.0 * torch.reciprocal(torch.exp(2.0 * x) + 1.0) if self.fn == "kernel" else torch.tanh(x)

    def _tra(self, v, pre):
        f = self.f
        e = (v * v).mean(dim=3)
        y = self._sum(F.conv1d, F.pad(e, [2, 0]), self.w[pre + ".depth_conv"], f[pre + ".depth_conv.bias"], groups=8)
        g = self._sigmoid(self._sum(F.conv1d, y, self.w[pre + ".point_conv"], f[pre + ".point_conv.bias"]))
        g = self._rnd(g, "gate_unrounded" if pre == "encoder.en_convs.3.tra" else None)
        return h16(v * g.unsqueeze(-1))

    def _gtconv(self, x, pre, deconv):
        f, w, b = self.f, self.w, self.b
        x1, x2 = x[:, :8], x[:, 8:]
        conv = F.conv_transpose2d if deconv else F.conv2d
        h = h16(F.prelu(self._sum(conv, x1, w[pre + ".point_conv1"], b[pre + ".point_conv1"]), f[pre + ".point_act.weight"]))
        if deconv:
            h = self._sum(F.conv_transpose2d, h, w[pre + ".depth_conv"], b[pre + ".depth_conv"], padding=(0, 1))[:, :, :x.shape[2]]
        else:
            hp, wd = F.pad(h, [0, 0, 2, 0]), w[pre + ".depth_conv"]
            h = self._sum(F.conv2d, hp, wd, b[pre + ".depth_conv"], padding=(0, 1), groups=16)
            if self.mutate == "stale_hist_16" and pre == "encoder.en_convs.2":
                wd = wd.clone()
                wd[:, :, :2] = 0.0                              # no history rows: what a lost chunk hand-off leaves
                h0 = self._sum(F.conv2d, hp, wd, b[pre + ".depth_conv"], padding=(0, 1), groups=16)
                h[:, :, 16::16] = h0[:, :, 16::16]
        h = h16(F.prelu(h, f[pre + ".depth_act.weight"]))
        v = self._sum(conv, h, w[pre + ".point_conv2"], b[pre + ".point_conv2"])
        if not (self.mutate == "no_round" and pre == "decoder.de_convs.1"):
            v = h16(v)
        v = self._tra(v, pre + ".tra")
        return torch.stack([v, x2], dim=2).flatten(1, 2)

    def _tcn(self, x, pre, d):
        f, w, b = self.f, self.w, self.b
        y = h16(F.prelu(self._sum(F.conv2d, x, w[pre + ".conv1"], b[pre + ".conv1"]), f[pre + ".act1.weight"]))
        y = self._sum(F.conv2d, F.pad(y, [0, 0, 2 * d, 0]), w[pre + ".conv2"], b[pre + ".conv2"], dilation=(d, 1), groups=16)
        y = self._rnd(F.prelu(y, f[pre + ".act2.weight"]), "tcn1_act2_unrounded" if pre == "gtcn1.blocks.2" else None)
        y = self._sum(F.conv2d, y, w[pre + ".conv3"], b[pre + ".conv3"])
        return self._rnd(F.prelu(y + x, f[pre + ".act3.weight"]), "tcn2_act3_unrounded" if pre == "gtcn2.blocks.0" else None)

    def _skip(self, x, skips, i):
        s = x + skips[i]
        return s if self.mutate == "skip_unrounded" and i == 3 else h16(s)

    @torch.inference_mode()
    def forward(self, spec, in_scale=0.0, out_scale=0.0, pins=None, taps=None):
        f, w, b = self.f, self.w, self.b
        away = self.mutate == "ties_away"

        def stage(name, x):
            """A stage boundary: hand the checker's value to `taps`, go on with the pinned one if there is one."""
            if taps is not None:
                taps[name] = x.float().contiguous().numpy().copy()
            if pins is not None and name in pins:
                x = torch.as_tensor(np.asarray(pins[name], np.float32)).to(self.dt)
            return x
        spec = torch.as_tensor(spec, dtype=torch.float32)
        if in_scale > 0:
            spec = int8_boundary(spec, in_scale, -127 if self.mutate == "clamp127" else -128, away)
        spec = h16(spec).to(self.dt)
        re, im = spec[..., 0].permute(0, 2, 1), spec[..., 1].permute(0, 2, 1)
        feat = torch.stack([self._rnd(torch.sqrt(re * re + im * im + 1e-12), "mag_unrounded"), re, im], dim=1)
        feat = torch.cat([feat[..., :65], h16(self._sum(F.linear, feat[..., 65:], w["erb"]))], dim=-1)
        x = h16(self._sum(F.conv2d, feat, w["sfe"], padding=(0, 1), groups=3))
        skips = []
        for i in range(2):
            pre = f"encoder.en_convs.{i}"
            x = self._sum(F.conv2d, x, w[pre + ".conv"], b[pre + ".conv"], stride=(1, 2), padding=(0, 2))
            x = self._rnd(F.prelu(x, f[pre + ".act.weight"]), "en1_unrounded" if i == 1 else None)
            x = stage(f"en{i}", x)
            skips.append(x)
        for i in range(2, 5):
            x = stage(f"en{i}", self._gtconv(x, f"encoder.en_convs.{i}", False))
            skips.append(x)
        for g in (1, 2):
            for k in range(4):
                x = self._tcn(x, f"gtcn{g}.blocks.{k}", 1 << k)
            if g == 1:
                x = stage("gtcn1", x)
        x = stage("sum4", self._skip(x, skips, 4))
        for i in range(3):
            x = stage(f"de{i}", self._gtconv(x, f"decoder.de_convs.{i}", True))
            x = self._skip(x, skips, 3 - i)
        pre = "decoder.de_convs.3"
        x = self._sum(F.conv_transpose2d, x, w[pre + ".conv"], b[pre + ".conv"], stride=(1, 2), padding=(0, 2))
        x = stage("de3", self._rnd(F.prelu(x, f[pre + ".act.weight"]), "de3_unrounded"))
        pre = "decoder.de_convs.4"
        m = self._sum(F.conv_transpose2d, self._skip(x, skips, 0), w[pre + ".conv"], b[pre + ".conv"], stride=(1, 2), padding=(0, 2))
        m = stage("de4", h16(self._tanh(m)))
        m = torch.cat([m[..., :65], self._rnd(self._sum(F.linear, m[..., 65:], w["ierb"]), "ierb_unrounded")], dim=-1)
        out = torch.stack([h16(re * m[:, 0] - im * m[:, 1]), h16(im * m[:, 0] + re * m[:, 1])], dim=-1).permute(0, 2, 1, 3)
        out = out.float()
        if out_scale > 0:
            out = int8_boundary(out, out_scale, ties_away=away)
        out = out.contiguous().numpy()
        if taps is not None:
            taps["out"] = out.copy()
        return out
