#!/usr/bin/env python3
"""Instruction mix of the offline kernels' gfx950 code, per kernel symbol.  Needs hipcc and c++filt, no GPU.

    python tools/valu_mix.py [--tree DIR] [--asm FILE] [--kernels REGEX] [--label TEXT]

Compiles DIR/gtcrn_micro_amd/csrc/kernels.hip (default: this tree) with the flags gtcrn_micro_amd/build.py uses for it
plus `-S --cuda-device-only`, or reads an assembly file made that way (--asm), splits it per kernel and prints, for the
offline instantiations of k_front, k_encoder, k_gtcn_band, k_decoder and k_istft, two rows each:

    fn    the whole function
    loop  its hot loop: the backward branch whose span holds the most matrix instructions (the chunk loop of
          k_gtcn_band / k_encoder / k_decoder, the frame loop of k_front); counts there are per trip and wave

Columns: MFMA; float VALU (any other vector instruction on a floating-point type, conversions included); integer /
move / select VALU (every remaining vector ALU instruction: address arithmetic, v_mov, v_cndmask, integer compares,
lane reads); LDS operations; global (and scratch) memory operations; scalar ALU, and of those the multiplies and
carry adds that 64-bit address formation and divisions are made of; s_nop; then the function's VGPRs and scratch bytes.

Why it matters: v_mfma_f32_16x16x4_f32 blocks the VALU while it runs, so in these kernels every vector instruction in a
steady-state loop is issue time that nothing hides.  The tool reports classes only.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-result", "-fno-honor-nans", "-ffp-contract=on"]
# the kernels an offline fixed-length batch launches (bench.py's workload) and the one-workgroup-per-time-span forms
DEFAULT = (r"^(?:void )?(?:\w+::)?(k_front<true, false>|k_encoder<3, false, false, false, (false|true)>|"
           r"k_gtcn_band<false, (false|true)>|k_decoder<false, 3, false, false, (false|true)>|k_istft)$")
FLOAT_T = re.compile(r"_(f16|f32|f64|bf16|fp8|bf8)\b|_(f16|f32|f64|bf16)_")
COLS = ("mfma", "fvalu", "ivalu", "lds", "glob", "salu", "smulc", "nop")


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return ("mfma",)
    if op.startswith("v_"):
        return ("fvalu",) if FLOAT_T.search(op) else ("ivalu",)
    if op.startswith("ds_"):
        return ("lds",)
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return ("glob",)
    if op == "s_nop":
        return ("nop",)
    if op.startswith("s_") and not op.startswith(("s_waitcnt", "s_cbranch", "s_branch", "s_barrier", "s_endpgm",
                                                  "s_load", "s_buffer_load", "s_sleep", "s_set", "s_code_end")):
        return ("salu", "smulc") if op.startswith(("s_mul", "s_addc", "s_subb")) else ("salu",)
    return ()


def count(ops):
    c = dict.fromkeys(COLS, 0)
    for op in ops:
        for k in classify(op):
            c[k] += 1
    return c


def functions(text):
    """name -> (list of (label or None, mnemonic, operand text), VGPRs, scratch bytes)"""
    out = {}
    for m in re.finditer(r"^(\S+):\s*; @\S+\n(.*?)^\.Lfunc_end\d+:(.*?)(?=^\S+:\s*; @|\Z)", text, re.S | re.M):
        body = []
        for ln in m.group(2).splitlines():
            ln = ln.split(";")[0].strip()
            if not ln:
                continue
            if re.match(r"^\.LBB\d+_\d+:", ln):
                body.append((ln[:-1], None, None))
            elif not ln.startswith("."):
                p = ln.split(None, 1)
                body.append((None, p[0], p[1] if len(p) > 1 else ""))
        meta = m.group(3)
        vg = re.search(r"; NumVgprs: (\d+)", meta)
        sc = re.search(r"; ScratchSize: (\d+)", meta)
        out[m.group(1)] = (body, int(vg.group(1)) if vg else -1, int(sc.group(1)) if sc else -1)
    return out


def hot_loop(body):
    """instructions between a label and the last backward branch to it; the span with the most MFMAs"""
    at = {}
    best, best_n = [], -1
    for i, (lab, op, args) in enumerate(body):
        if lab:
            at[lab] = i
        elif op.startswith(("s_cbranch", "s_branch")) and args.strip() in at:
            span = [o for (_, o, _) in body[at[args.strip()]:i + 1] if o]
            n = sum(1 for o in span if o.startswith("v_mfma"))
            # ties: the first to close (an inner loop closes before the one around it, and before the out-of-line
            # blocks behind the loop that branch back into it); a kernel without MFMA: its longest loop
            if n > best_n or (n == 0 and best_n == 0 and len(span) > len(best)):
                best, best_n = span, n
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="source tree whose kernels.hip is compiled")
    ap.add_argument("--asm", default=None, help="read this assembly file instead of compiling")
    ap.add_argument("--kernels", default=DEFAULT, help="regex on the demangled name without its argument list")
    ap.add_argument("--label", default=None, help="heading printed above the table")
    a = ap.parse_args()
    if a.asm:
        text = open(a.asm).read()
    else:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        with tempfile.TemporaryDirectory() as tmp:
            s = os.path.join(tmp, "kernels.s")
            subprocess.check_call([hipcc, "--offload-arch=gfx950"] + FLAGS + ["--cuda-device-only", "-S",
                                  os.path.join(a.tree, "gtcrn_micro_amd", "csrc", "kernels.hip"), "-o", s])
            text = open(s).read()
    fns = functions(text)
    names = list(fns)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    rows = sorted((re.sub(r"\(.*$", "", d), n) for d, n in zip(dem, names))
    pat = re.compile(a.kernels)
    if a.label:
        print(a.label)
    print(f"{'kernel':58s} {'part':4s} " + " ".join(f"{c:>6s}" for c in COLS) + "  VGPRs scratch")
    hit = 0
    for d, n in rows:
        if not pat.search(d):
            continue
        hit += 1
        body, vg, sc = fns[n]
        for part, ops in (("fn", [o for (_, o, _) in body if o]), ("loop", hot_loop(body))):
            c = count(ops)
            print(f"{re.sub(r'^void ', '', d) if part == 'fn' else '':58s} {part:4s} " + " ".join(f"{c[k]:6d}" for k in COLS) +
                  (f"  {vg:5d} {sc:7d}" if part == "fn" else ""))
    if not hit:
        print("no kernel matches", a.kernels, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
