"""Builds the gfx950 shared library in-tree (gtcrn_micro_amd/libgtcrn_micro_hip.so).

hipcc cross-compiles for gfx950 without a GPU; the .so travels with the repo
snapshot to the GPU box.  No CPU fallback is built: the library is HIP only.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libgtcrn_micro_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCES = ["kernels.hip", "api.cpp", "pack.cpp", "train_kernels.hip", "train.cpp", "metrics.hip", "metrics_host.cpp", "batch.hip", "batch_host.cpp", "reverb.hip", "reverb_host.cpp", "phone.hip", "phone_host.cpp", "mixer.hip", "mixer_host.cpp", "plc.hip", "plc_host.cpp"]
HEADERS = ["kernels.h", "fft256.h", "stream_ms_body.inc", "layout.h", "pack.h", "train_kernels.h", "metrics.h", "batch.h", "reverb.h", "phone.h", "mixer.h", "plc.h", os.path.join("..", "..", "include", "gtcrn_micro_hip.h")]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_native(force=False, verbose=False, stamps=False, exp=False):
    """stamps=True builds the diagnostic variant libgtcrn_micro_hip_stamps.so (-DGT_STAMPS: in-kernel
    s_memtime phase stamps, used only by tools/phase_profile.py; never loaded by the product path).
    exp=True builds libgtcrn_micro_hip_exp.so with -DGT_EXP: whatever kernel experiment currently sits behind
    `#ifdef GT_EXP`, timed against the default build on the same GPU by tools/ab_bench.py."""
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS] + [os.path.abspath(__file__)]   # the flags live here
    objs = []
    common = ["-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-result"]
    # Inference kernels (kernels.hip):
    #  -fno-honor-nans: keeps hipcc from canonicalising (v_max x,x) in front of every v_min/v_max of the PReLU; no
    #     kernel tests for or produces NaN on finite input.  The level control's block rule (kernels.h, alc_decide) has to
    #     survive a NaN or Inf in a stream under this flag: its finiteness test reads the bits (alc_not_finite), and it needs
    #     only that a NaN passes through the adds and multiplies of the reductions, which the flag does not change.  It also
    #     relies on hipcc's default correctly rounded fp32 `/` and sqrt (-fhip-fp32-correctly-rounded-divide-sqrt): do not
    #     add -ffast-math or -fno-hip-fp32-correctly-rounded-divide-sqrt here (tests/test_gpu_alc.py compares bit for bit).
    #  -ffp-contract=on: multiply-adds are fused per source expression (by the front end), not opportunistically by the
    #     back end: every instantiation of a kernel template (one/two/three tiles per wave, offline / streaming /
    #     multi-stream) then rounds identically, which is what makes streamed == chunked == offline hold BIT FOR BIT.
    # Training kernels keep the defaults: NaN/Inf of a diverged run must propagate, and their fp32 statistics are
    # measurably more accurate with the back end's contraction (tests/test_gpu_train.py, fp64 comparison).
    # Batch kernels (batch.hip, and the plan's host twin in batch_host.cpp): -ffp-contract=off, because their contract is
    #     stated operation by operation (a rounded multiply, then a rounded add) and numpy restates it bit for bit.
    # Reverb kernels (reverb.hip, reverb_host.cpp): integer arithmetic but for the reverb plan's one float compare; the same
    #     flag, so that the plan's body is compiled as the batch plan's is.
    # Phone kernels (phone.hip, phone_host.cpp): integer arithmetic but for one exact multiply per sample and the phone plan's one
    #     float compare; the same flag, for the same reason.
    # Mixer kernels (mixer.hip, mixer_host.cpp): -ffp-contract=off, because the conference mix is stated as single rounded fp32
    #     operations in a fixed order (tests/mixer_checker.py restates it bit for bit).  Its fade ramp fl(fl(i + 1) / fl(n)) relies
    #     on hipcc's default correctly rounded fp32 `/` (-fhip-fp32-correctly-rounded-divide-sqrt): do not add -ffast-math or
    #     -fno-hip-fp32-correctly-rounded-divide-sqrt to these files.
    # Concealment kernels (plc.hip, plc_host.cpp): -ffp-contract=off, because the contract is single stated operations: the lag
    #     search's score is one rounded product and one rounded quotient in double, the float cross-fade two rounded products and
    #     a rounded sum, and everything else is integer arithmetic (tests/plc_checker.py restates it bit for bit).
    per_file = {"kernels.hip": ["-fno-honor-nans", "-ffp-contract=on"], "batch.hip": ["-ffp-contract=off"],
                "batch_host.cpp": ["-ffp-contract=off"], "reverb.hip": ["-ffp-contract=off"],
                "reverb_host.cpp": ["-ffp-contract=off"], "phone.hip": ["-ffp-contract=off"],
                "phone_host.cpp": ["-ffp-contract=off"], "mixer.hip": ["-ffp-contract=off"],
                "mixer_host.cpp": ["-ffp-contract=off"], "plc.hip": ["-ffp-contract=off"],
                "plc_host.cpp": ["-ffp-contract=off"]}
    suffix = ""
    lib = LIB
    if stamps:
        common.append("-DGT_STAMPS")
        per_file = {k: v + os.environ.get("GT_STAMPS_FLAGS", "").split() for k, v in per_file.items()}
        suffix = ".stamps"
        lib = LIB.replace(".so", "_stamps.so")
    elif exp:
        common.append("-DGT_EXP")
        per_file = {k: v + os.environ.get("GT_EXP_FLAGS", "").split() for k, v in per_file.items()}
        suffix = ".exp"
        lib = LIB.replace(".so", "_exp.so")
    for src in SOURCES:
        obj = os.path.join(CSRC, os.path.splitext(src)[0] + suffix + ".o")
        objs.append(obj)
        if force or _stale(obj, deps):
            cmd = [HIPCC, "--offload-arch=gfx950"] + common + per_file.get(src, []) + ["-c", os.path.join(CSRC, src), "-o", obj]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
    if force or _stale(lib, objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return lib


if __name__ == "__main__":
    print(build_native(verbose=True))
