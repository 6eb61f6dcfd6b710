"""Functional PyTorch-CPU port of the GTCRN-Micro hot path (test infrastructure + CPU baseline).

TEST INFRASTRUCTURE ONLY, like everything under oracle/: never imported by the product.
Why it exists next to the C oracle: the reference executes on PyTorch ATen (mkldnn conv,
native BN/PReLU, pocketfft), and its Python cannot travel to the GPU box.  This port issues the
same ATen op sequence from the flat parameter blob, so that bench.py's `cpu_baseline` times the
reference's own CPU arithmetic (kind "port") rather than a slower scalar restatement.
Parity status: PINNED against tests/golden (tests/test_oracle_golden.py).

Written from the layer list in SURVEY.md section 2a / Appendix A; cites reference lines.
"""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

_HERE = os.path.dirname(os.path.abspath(__file__))
_MANIFEST = os.path.join(_HERE, "..", "tests", "golden", "params_manifest.json")


def blob_to_dict(blob):
    man = json.load(open(_MANIFEST))
    blob = np.asarray(blob, np.float32)
    return {n: torch.from_numpy(blob[o:o + int(np.prod(s))].reshape(s).copy()) for n, s, o in man["tensors"]}


def is_trainable(name):
    """The 248 tensors train.py hands to Adam: everything except BatchNorm running statistics and the
    frozen ERB filterbank (models/gtcrn_micro.py:27-33, requires_grad False)."""
    return not (name.endswith("running_mean") or name.endswith("running_var") or name.startswith("erb."))


class _RoundSTE(torch.autograd.Function):
    """x -> bf16(x) (round to nearest even) with a straight-through gradient: what a tensor STORED in bf16 and read
    back by its consumers looks like to the rest of the graph."""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


class _GradRoundBF16(torch.autograd.Function):
    """Identity forward; the gradient is rounded to bf16 on its way back: a gradient tensor the trainer hands from one
    unit to the next in bf16 (storage "bf16_grads", csrc/train.cpp gtcrn_train_backward / unit_bwd `gbf`)."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


class TorchPort:
    def __init__(self, blob, train=False, dtype=torch.float32, store=None, pin=None, grad_round=False):
        """train=True: BatchNorm uses batch statistics and updates the running ones in place
        (nn.BatchNorm2d in .train() mode, momentum 0.1), and trainable tensors require grad.
        dtype=torch.float64 runs the same graph in double: the "truth" that fp32 results scatter around.
        store="bf16": the graph of the HIP trainer's bf16 storage mode (BASELINE configs[3]) -- every tensor the
        trainer writes out (features, conv outputs centred on the running mean, activations, block outputs, decoder
        sums, the mask) is rounded to bf16 where it is produced and its consumers read the rounded value; arithmetic in
        `dtype`.  With dtype=float64 this is the truth for THAT network: bf16-activation training computes the
        gradient of a slightly different function than the fp32 network (tests/reports/bf16_storage_ablation.py).
        pin: {name: tensor (B,C,T,F)} -- at every point the trainer stores (the names of gtcrn_train_tap: the centred
        conv output "<bn prefix>.y" of every unit inside _bn, the block outputs en0..en4 / tcn0..tcn7 / gtcn1, gtcn2 /
        de0..de4, the decoder sums sum0..sum4) the value is replaced by the pinned one through a straight-through snap,
        v + (pin - v).detach(): every unit then sees exactly the inputs the trainer's unit saw (no compounding of rounding
        flips along the chain) and the gradient still flows through this graph.  `skips` keep the pinned values.
        grad_round=True (with store="bf16"): the gradient is rounded to bf16 at every hand-off the trainer stores in bf16
        in storage "bf16_grads" (activations, block outputs, decoder sums, the TCN residual; not the mask's or the SFE
        output's gradient, which stay fp32)."""
        self.pin = pin
        self.grad_round = bool(grad_round)
        self._taps = None
        self.p = {k: v.to(dtype) for k, v in blob_to_dict(blob).items()}
        self.dtype = dtype
        self.store = store
        self.train = bool(train)
        if self.train:
            for k, v in self.p.items():
                if is_trainable(k):
                    v.requires_grad_(True)

    # conv + BatchNorm + activation (ConvBlock.forward, models/gtcrn_micro.py:163-164)
    def _r(self, x, grad=True):
        if self.store != "bf16":
            return x
        x = _RoundSTE.apply(x)
        return self._gr(x) if grad else x

    def _gr(self, x):
        return _GradRoundBF16.apply(x) if self.grad_round else x

    def _pt(self, name, v):
        """A stored tensor: recorded (its value BEFORE any pin) when taps are asked for, then snapped to the pin."""
        if self._taps is not None:
            self._taps[name] = v.detach().clone()
        if self.pin is not None and name in self.pin:
            v = v + (torch.as_tensor(self.pin[name]).to(v.dtype) - v).detach()
        return v

    def _bn(self, x, pre):
        p = self.p
        if self.store == "bf16":
            # the conv output is stored centred on the channel's mean of the previous step (the running mean before the
            # first one, csrc/train.cpp unit_fwd); the batch statistics are taken from the stored values
            rm = p[pre + ".running_mean"].detach().clone().view(1, -1, 1, 1)
            x = self._pt(pre + ".y", _RoundSTE.apply(x - rm)) + rm
        else:
            x = self._pt(pre + ".y", x)
        return F.batch_norm(x, p[pre + ".running_mean"], p[pre + ".running_var"], p[pre + ".weight"],
                            p[pre + ".bias"], self.train, 0.1, 1e-5)

    def _tra(self, x, pre):
        # TRALite.forward (models/gtcrn_micro.py:122-139), zero cache
        p = self.p
        e = (x * x).mean(dim=3)
        y = F.conv1d(F.pad(e, [2, 0]), p[pre + ".depth_conv.weight"], p[pre + ".depth_conv.bias"], groups=8)
        g = torch.sigmoid(F.conv1d(y, p[pre + ".point_conv.weight"], p[pre + ".point_conv.bias"]))
        return x * g.unsqueeze(-1)

    def _gtconv(self, x, pre, deconv):
        # GTConvBlock.forward (models/gtcrn_micro.py:229-253)
        p = self.p
        x1, x2 = x[:, :8], x[:, 8:]
        conv = F.conv_transpose2d if deconv else F.conv2d
        h = conv(x1, p[pre + ".point_conv1.weight"], p[pre + ".point_conv1.bias"])
        h = self._r(F.prelu(self._bn(h, pre + ".point_bn1"), p[pre + ".point_act.weight"]))
        if deconv:
            h = F.conv_transpose2d(h, p[pre + ".depth_conv.weight"], p[pre + ".depth_conv.bias"], padding=(0, 1))
        else:
            h = F.conv2d(F.pad(h, [0, 0, 2, 0]), p[pre + ".depth_conv.weight"], p[pre + ".depth_conv.bias"],
                         padding=(0, 1), groups=16)
        h = self._r(F.prelu(self._bn(h, pre + ".depth_bn"), p[pre + ".depth_act.weight"]))
        h = self._r(self._bn(conv(h, p[pre + ".point_conv2.weight"], p[pre + ".point_conv2.bias"]), pre + ".point_bn2"))
        h = self._tra(h, pre + ".tra")[:, :, :x2.shape[2]]
        return self._r(torch.stack([h, x2], dim=2).flatten(1, 2))      # out[2c] = h[c], out[2c+1] = x2[c]

    def _tcn(self, x, pre, d):
        # TCN.forward (models/gtcrn_micro.py:290-310)
        p = self.p
        y = self._r(F.prelu(self._bn(F.conv2d(x, p[pre + ".conv1.weight"], p[pre + ".conv1.bias"]), pre + ".bn1"),
                            p[pre + ".act1.weight"]))
        y = F.conv2d(F.pad(y, [0, 0, 2 * d, 0]), p[pre + ".conv2.weight"], p[pre + ".conv2.bias"],
                     dilation=(d, 1), groups=16)
        y = self._r(F.prelu(self._bn(y, pre + ".bn2"), p[pre + ".act2.weight"]))
        y = self._bn(F.conv2d(y, p[pre + ".conv3.weight"], p[pre + ".conv3.bias"]), pre + ".bn3")
        return self._r(F.prelu(y + self._gr(x), p[pre + ".act3.weight"]))      # (the residual's gradient: a hand-off)

    def forward(self, spec, taps=None):
        """GTCRNMicro.forward (models/gtcrn_micro.py:506-532): (B,257,T,2) -> (B,257,T,2)."""
        if self.train:
            return self._forward(spec, taps)
        with torch.inference_mode():
            return self._forward(spec, taps)

    def _forward(self, spec, taps=None):
        self._taps = taps
        try:
            return self._forward_body(spec)
        finally:
            self._taps = None

    def _forward_body(self, spec):
        p = self.p
        tap = self._pt
        spec = torch.as_tensor(spec).to(self.dtype)
        re, im = spec[..., 0].permute(0, 2, 1), spec[..., 1].permute(0, 2, 1)
        feat = torch.stack([torch.sqrt(re * re + im * im + 1e-12), re, im], dim=1)
        feat = self._r(torch.cat([feat[..., :65], F.linear(feat[..., 65:], p["erb.erb_fc.weight"])], dim=-1), False)
        x = self._r(F.conv2d(feat, p["sfe.depth_conv.weight"], padding=(0, 1), groups=3), False)   # (df0: fp32)
        skips = []
        for i in range(2):
            pre = f"encoder.en_convs.{i}"
            x = F.conv2d(x, p[pre + ".conv.weight"], p[pre + ".conv.bias"], stride=(1, 2), padding=(0, 2))
            x = tap(f"en{i}", self._r(F.prelu(self._bn(x, pre + ".bn"), p[pre + ".act.weight"])))
            skips.append(x)
        for i in range(2, 5):
            x = tap(f"en{i}", self._gtconv(x, f"encoder.en_convs.{i}", False))
            skips.append(x)
        for g in (1, 2):
            for k in range(4):
                x = tap(f"tcn{4 * g - 4 + k}", self._tcn(x, f"gtcn{g}.blocks.{k}", 1 << k))
            x = tap(f"gtcn{g}", x)
        for i in range(3):
            x = tap(f"de{i}", self._gtconv(tap(f"sum{i}", self._r(x + skips[4 - i])), f"decoder.de_convs.{i}", True))
        pre = "decoder.de_convs.3"
        x = F.conv_transpose2d(tap("sum3", self._r(x + skips[1])), p[pre + ".conv.weight"], p[pre + ".conv.bias"],
                               stride=(1, 2), padding=(0, 2))
        x = tap("de3", self._r(F.prelu(self._bn(x, pre + ".bn"), p[pre + ".act.weight"])))
        pre = "decoder.de_convs.4"
        x = F.conv_transpose2d(tap("sum4", self._r(x + skips[0])), p[pre + ".conv.weight"], p[pre + ".conv.bias"],
                               stride=(1, 2), padding=(0, 2))
        m = tap("de4", self._r(torch.tanh(self._bn(x, pre + ".bn")), False))      # (dm: fp32)
        m = torch.cat([m[..., :65], F.linear(m[..., 65:], p["erb.ierb_fc.weight"])], dim=-1)   # (B,2,T,257)
        out_re = re * m[:, 0] - im * m[:, 1]
        out_im = im * m[:, 0] + re * m[:, 1]
        return torch.stack([out_re, out_im], dim=-1).permute(0, 2, 1, 3)

    # ---- train step (train.py:239-288): HybridLoss (loss.py:30-71) and the gradients ----------------
    @staticmethod
    def hybrid_loss(pred, true):
        pr, pi, tr, ti = pred[..., 0], pred[..., 1], true[..., 0], true[..., 1]
        pm = torch.sqrt(pr ** 2 + pi ** 2 + 1e-12)
        tm = torch.sqrt(tr ** 2 + ti ** 2 + 1e-12)
        mse = F.mse_loss
        ri = mse(pr / pm ** 0.7, tr / tm ** 0.7) + mse(pi / pm ** 0.7, ti / tm ** 0.7)
        mag = mse(pm ** 0.3, tm ** 0.3)
        win = torch.hann_window(512).pow(0.5).to(pred.device)
        yp = torch.istft(torch.complex(pr, pi), 512, 256, 512, window=win)
        yt = torch.istft(torch.complex(tr, ti), 512, 256, 512, window=win)
        yt = torch.sum(yt * yp, -1, keepdim=True) * yt / (torch.sum(yt ** 2, -1, keepdim=True) + 1e-8)
        sisnr = -torch.log10(torch.norm(yt, dim=-1, keepdim=True) ** 2 /
                             (torch.norm(yp - yt, dim=-1, keepdim=True) ** 2 + 1e-8) + 1e-8).mean()
        return 30 * ri + 70 * mag + sisnr

    def blob(self):
        man = json.load(open(_MANIFEST))
        return np.concatenate([self.p[n].detach().numpy().astype(np.float32).ravel() for n, _, _ in man["tensors"]])

    def grads_blob(self):
        """d loss / d parameter in the canonical blob layout (zeros in the slots of buffers)."""
        man = json.load(open(_MANIFEST))
        out = []
        for n, s, _ in man["tensors"]:
            g = self.p[n].grad
            out.append((g if g is not None else torch.zeros(s)).detach().numpy().astype(np.float32).ravel())
        return np.concatenate(out)

    def train_step(self, noisy_spec, clean_spec):
        """One forward/backward in train mode; returns (enh, loss, d loss/d enh, grads blob)."""
        assert self.train
        for v in self.p.values():
            v.grad = None
        enh = self.forward(torch.as_tensor(noisy_spec, dtype=torch.float32))
        enh.retain_grad()
        loss = self.hybrid_loss(enh, torch.as_tensor(clean_spec, dtype=torch.float32))
        loss.backward()
        return enh.detach().numpy(), float(loss), enh.grad.numpy(), self.grads_blob()

    def backward_from(self, spec, grad_enh, taps=None):
        """Gradients for a given upstream gradient (the model's backward alone, without the loss).  taps: a dict that
        receives every stored tensor of the forward by its gtcrn_train_tap name (values before any pin)."""
        assert self.train
        for v in self.p.values():
            v.grad = None
        enh = self.forward(torch.as_tensor(spec).to(self.dtype), taps)
        enh.backward(torch.as_tensor(grad_enh).to(self.dtype))
        return enh.detach().numpy(), self.grads_blob()

    @torch.inference_mode()
    def enhance(self, wave, window):
        """infer.py:60-76 for a batch of equal-length clips (the caller loop of the reference)."""
        wave = torch.as_tensor(wave, dtype=torch.float32)
        window = torch.as_tensor(window, dtype=torch.float32)
        spec = torch.view_as_real(torch.stft(wave, 512, 256, 512, window, return_complex=True))
        out = self.forward(spec)
        return torch.istft(torch.view_as_complex(out.contiguous()), 512, 256, 512, window)
