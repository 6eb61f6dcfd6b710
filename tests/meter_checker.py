"""Checker of the level meters (include/gtcrn_micro_hip.h, "level meters").

A stream's record {E_dry, E_out, peak, blocks} is checked against float64 sums of the blocks the stream emitted and of the
dry blocks aligned with them.  The caller passes, per emitted block, the 256 floats handed to the store (before any int16
rounding) and the 256 dry samples of the contract -- zeros for a structural zero block (the first hop of a stream, the
flush of a stream that holds fewer than 257 samples), whose emitted block is zeros too.

Acceptance: blocks equal, peak bit-equal, and each energy within the textbook bound of a sum of non-negative terms,
    |E - E64| <= b E64,   b = m u / (1 - m u),   u = 2^-24,   m = D + K + 1,
K the hops accumulated since the records were zeroed and D the depth of the in-wave reduction order, READ from the
header.  The bound is derived, not measured: every term passes at most D roundings (its square, the adds of the lane
partial and of the butterfly) and K accumulating adds, each a factor (1 + d), |d| <= u, on a sum whose terms are all >= 0.

`emulate` is the header's order in numpy float32 (lane partials, butterfly, sequential hops): it reproduces a device record
bit for bit and is what the seeded-bug tests distort."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
F32 = np.float32


def header_depth():
    """D as include/gtcrn_micro_hip.h states it (a line `*     D = <number>` of the "level meters" section)."""
    with open(os.path.join(ROOT, "include", "gtcrn_micro_hip.h")) as f:
        text = f.read()
    sec = text[text.index("level meters:"):]
    m = re.search(r"^ \*\s+D = (\d+)\s*$", sec, re.M)
    assert m, "the header states no depth D"
    d = int(m.group(1))
    assert 1 <= d <= 16, d
    return d


def bound(K, D=None):
    m = (header_depth() if D is None else D) + int(K) + 1
    return m * U / (1.0 - m * U)


def _blocks(a):
    a = np.asarray(a)
    assert a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 256, (a.dtype, a.shape)
    return a


def reference(out_blocks, dry_blocks, hops=None, start=None):
    """float64 energies, exact peak (float32) and block count after the blocks `hops` (indices into the (K, 256) arrays, in
    order; None: all of them), starting from the record `start` (None: zeros)."""
    out_blocks, dry_blocks = _blocks(out_blocks), _blocks(dry_blocks)
    hops = range(len(out_blocks)) if hops is None else list(hops)
    s = np.zeros(4, np.float32) if start is None else np.asarray(start, np.float32)
    e_dry, e_out, peak, blocks = float(s[0]), float(s[1]), F32(s[2]), float(s[3])
    for h in hops:
        e_dry += float(np.sum(dry_blocks[h].astype(np.float64) ** 2))
        e_out += float(np.sum(out_blocks[h].astype(np.float64) ** 2))
        peak = max(peak, F32(np.max(np.abs(out_blocks[h]))))
        blocks += 1.0
    return e_dry, e_out, F32(peak), blocks


def problems(record, out_blocks, dry_blocks, hops=None, start=None, K=None):
    """The list of what is wrong with `record` (4 float32 values); empty: accepted.  K: hops accumulated since the records
    were zeroed (default: the blocks of `start` plus the hops given here)."""
    rec = np.asarray(record, np.float32).reshape(4)
    e_dry, e_out, peak, blocks = reference(out_blocks, dry_blocks, hops, start)
    if K is None:
        K = int(blocks)
    b = bound(K)
    bad = []
    if float(rec[3]) != blocks:
        bad.append(f"blocks {float(rec[3])} != {blocks}")
    if rec[2:3].view(np.uint32)[0] != np.array([peak], np.float32).view(np.uint32)[0]:
        bad.append(f"peak {rec[2]!r} != {peak!r}")
    for name, got, want in (("E_dry", float(rec[0]), e_dry), ("E_out", float(rec[1]), e_out)):
        err = abs(got - want)
        if not err <= b * want:
            bad.append(f"{name} {got!r} against {want!r}: |err| {err:.3e} > {b * want:.3e} (K = {K})")
    return bad


def check(record, out_blocks, dry_blocks, hops=None, start=None, K=None, what=""):
    bad = problems(record, out_blocks, dry_blocks, hops, start, K)
    assert not bad, (what, bad)


# ------------------------------------------------------------------------------------------- the stated order, float32
def hop_sum(block):
    """e_h of one 256-sample block: lane l holds samples 2l, 2l+1, 128+2l, 129+2l, p = ((s0^2 + s1^2) + s2^2) + s3^2, then
    the xor butterfly over lane distances 1, 2, 4, 8, 16, 32; every operation one float32 rounding."""
    b = np.asarray(block, np.float32)
    sq = (b * b).astype(np.float32)
    lane = np.arange(64)
    p = (sq[2 * lane] + sq[2 * lane + 1]).astype(np.float32)
    p = (p + sq[128 + 2 * lane]).astype(np.float32)
    p = (p + sq[129 + 2 * lane]).astype(np.float32)
    for d in (1, 2, 4, 8, 16, 32):
        p = (p + p[lane ^ d]).astype(np.float32)
    assert (p.view(np.uint32) == p.view(np.uint32)[0]).all()
    return p[0]


def emulate(out_blocks, dry_blocks, hops=None, start=None):
    """The record after the blocks `hops` in the header's order: acc = fl(acc + e_h), hop after hop."""
    out_blocks, dry_blocks = _blocks(out_blocks), _blocks(dry_blocks)
    hops = range(len(out_blocks)) if hops is None else list(hops)
    rec = np.zeros(4, np.float32) if start is None else np.array(start, np.float32).reshape(4)
    for h in hops:
        rec[0] = F32(rec[0] + hop_sum(dry_blocks[h]))
        rec[1] = F32(rec[1] + hop_sum(out_blocks[h]))
        rec[2] = max(rec[2], F32(np.max(np.abs(out_blocks[h]))))
        rec[3] = F32(rec[3] + F32(1))
    return rec


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())
