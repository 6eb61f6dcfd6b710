// train_kernels.hip -- gfx950 kernels of the train-mode forward/backward (see train_kernels.h).
//
// The training row is layer-at-a-time (train-mode BatchNorm needs whole-batch
// statistics between layers), so every pass streams channels-last tensors through HBM once: dense convs,
// their data gradients and weight gradients on the fp32 matrix cores, everything else as 16-byte-per-lane
// streaming kernels; reductions are two-stage with a fixed summation order (per-thread fp32 over a bounded
// run, then double): bit-reproducible gradients, no atomics.
// Reference semantics are cited per kernel (paths relative to the reference repo).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "train_kernels.h"

namespace gtt {

namespace {

constexpr int NT = 256;
typedef float f32x4 __attribute__((ext_vector_type(4)));

inline int grid_for(long n, int cap = 4096) {
    long g = (n + NT - 1) / NT;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

// XCD-aware workgroup numbering for the grid-stride kernels that read temporal taps: the hardware deals workgroups
// round-robin to the 8 XCDs (each with its own L2), so with the plain blockIdx the rows t - d, t + d a thread needs
// were fetched by workgroups on OTHER XCDs and every line crossed the fabric three times.  With this numbering XCD x
// sweeps one contiguous eighth of each grid-stride window and the taps hit its own L2.
__device__ __forceinline__ unsigned xcd_block() {
    const unsigned b = blockIdx.x, n = gridDim.x;
    return (n & 7u) == 0 ? (b & 7u) * (n >> 3) + (b >> 3) : b;
}

// ------------------------------------------------------------------ in-launch finish of the two-stage reductions
// Every BatchNorm of a step needs two whole-batch reductions (forward: sum y, sum y^2; backward: sum dz, sum dz xhat, the
// slope terms).  Their first stage runs inside a streaming kernel (per-workgroup sums of K <= 48 doubles); the second
// stage used to be a kernel of its own -- 92 launches of 9-11 us per step, one 1024-thread workgroup each, almost all of
// it load latency over up to 1 024 partials (profiles/r04_train_f32_kernel_stats.csv: k_bn_stats_finish 46 x 11.3 us,
// k_bn_bwd_finish 46 x 9.5 us: 0.96 ms of a 30 ms step for 0.3 MB of data).  Now the LAST workgroup to finish does it,
// in two levels so that no workgroup reads more than 32 partials (one latency round of eight loads per thread):
//   level 1  workgroups are numbered in groups of FIN_G = 32; the last arriver of a group (a ticket from the group's
//            counter) adds the group's partials -- in index order, the arrival order does not enter the result -- into
//            one group sum;
//   level 2  the last group to finish (a ticket from the launch's counter) adds the <= 32 group sums and evaluates the
//            finish (statistics + running estimates, or the backward's means and parameter gradients).
// Hand-off between workgroups (cdna_hip_programming.md, guideline 16, counter form): partials and group sums are stored
// write-through (agent-scope relaxed atomic stores = sc1) by wave 0, which drains them (s_waitcnt vmcnt(0)) before its
// lane 0 takes the ticket (agent-scope relaxed fetch_add); the reducer reads them with agent-scope relaxed atomic loads
// (sc1: never from its CU's L1).  No fence, no spin.  The counters are zero between launches: the last arrivers reset
// them, the trainer zeroes them when it is created and at the start of every forward / backward call.
// Results are bit-reproducible (fixed order) and equal the former finish kernels' to the last bit of the float they
// produce except where a double sum rounds differently in its 53rd bit -- the fusion tests compare forwards bit for bit.
constexpr int FIN_G = 32;            // workgroups per group
constexpr int FIN_GROUPS = 32;       // MAX_PARTIALS / FIN_G
static_assert(FIN_G * FIN_GROUPS >= MAX_PARTIALS, "group table too small");
struct FinArgs {
    int kind;                        // 0: off (the host launches the finish kernel), 1: forward statistics, 2: backward
    int C;
    long n;
    double* gpart;                   // [FIN_GROUPS][64]
    unsigned* ctr;                   // [0]: groups finished, [1 + g]: workgroups of group g finished
    float *o0, *o1, *o2, *o3, *o4;   // kind 1: stats, running_mean, running_var, shift, stats_b; kind 2: red, dgamma, dbeta, dslope
};
typedef __attribute__((address_space(1))) unsigned long long gu64_t;
typedef __attribute__((address_space(1))) unsigned gu32_t;
__device__ __forceinline__ void st_pub(double* p, double v) {
    __hip_atomic_store((gu64_t*)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_pub(const double* p) {
    return __longlong_as_double((long long)__hip_atomic_load((gu64_t*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
// statistics of a train-mode BatchNorm from tot[0..C) = sum y, tot[C..2C) = sum y^2 (threads c < C)
__device__ __forceinline__ void bn_stats_math(const double* tot, long n, int C, float* stats, float* rmean, float* rvar,
                                              float* shift, float* stats_b) {
    const int c = threadIdx.x;
    if (c >= C) return;
    const double mean = tot[c] / (double)n;
    double var = tot[C + c] / (double)n - mean * mean;
    if (var < 0.0) var = 0.0;
    stats[c] = (float)mean;
    stats[C + c] = (float)(1.0 / sqrt(var + 1e-5));
    if (stats_b) {
        // exact chain: the backward's 16-bit copy of this tensor is written by its consumer as bf16(y - stats[c]):
        // centred on THIS step's mean, so the backward's statistics for it are mean 0 and the same invstd
        stats_b[c] = 0.f;
        stats_b[C + c] = stats[C + c];
    }
    if (rmean) {
        const double unb = n > 1 ? var * (double)n / (double)(n - 1) : var;
        // shift: the tensor holds y - shift[c], so mean(y) = mean + shift[c]; that becomes the next step's shift
        const double absmean = (shift && !stats_b) ? mean + (double)shift[c] : mean;
        rmean[c] = (float)(0.9 * (double)rmean[c] + 0.1 * absmean);
        if (shift) shift[c] = (float)absmean;
        rvar[c] = (float)(0.9 * (double)rvar[c] + 0.1 * unb);
    }
}
// first backward pass of a BatchNorm from tot[0..C) = sum dz, tot[C..2C) = sum dz xhat, tot[2C..3C) = slope terms
__device__ __forceinline__ void bn_bwd_math(const double* tot, long n, int C, float* red, float* dgamma, float* dbeta,
                                            float* dslope) {
    const int c = threadIdx.x;
    if (c < C) {
        red[c] = (float)(tot[c] / (double)n);
        red[C + c] = (float)(tot[C + c] / (double)n);
        if (dgamma) dgamma[c] = (float)tot[C + c];
        if (dbeta) dbeta[c] = (float)tot[c];
    }
    if (c == 0 && dslope) {
        double t = 0.0;
        for (int i = 0; i < C; ++i) t += tot[2 * C + i];
        dslope[0] = (float)t;
    }
}
// sum over q = sl, sl + 4, ... < cnt of src[q * stride + j] (j < K), eight loads in flight, fixed order
__device__ __forceinline__ double fin_gather(const double* src, int stride, int cnt, int j, int K, int sl) {
    const int jj = j < K ? j : K - 1;
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int q = sl + 4 * u;
        v[u] = ld_pub(src + (long)(q < cnt ? q : cnt - 1) * stride + jj);     // clamped: a valid element, not summed
    }
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) s += (sl + 4 * u < cnt) ? v[u] : 0.0;
    return s;
}
// Called by EVERY thread of the workgroup, as its last action, after threads tid < K (wave 0) have stored
// partial[vb * K + tid] with st_pub.  vb: this workgroup's index in [0, nblk) (any bijection of blockIdx.x).
__device__ __forceinline__ void fin_reduce(const double* partial, int K, int vb, int nblk, const FinArgs& fa) {
    __shared__ double f_sh[NT / 64][64];
    __shared__ double f_tot[64];
    __shared__ unsigned f_tk;
    const int tid = threadIdx.x, j = tid & 63, sl = tid >> 6;
    const int grp = vb / FIN_G, ngrp = (nblk + FIN_G - 1) / FIN_G, g0 = grp * FIN_G;
    const int gsz = nblk - g0 < FIN_G ? nblk - g0 : FIN_G;
    if (tid < 64) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // wave 0's partial has left the CU (sc1 stores)
        if (tid == 0) f_tk = __hip_atomic_fetch_add((gu32_t*)(fa.ctr + 1 + grp), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (f_tk != (unsigned)(gsz - 1)) return;                      // (uniform) not the group's last arriver
    f_sh[sl][j] = fin_gather(partial + (long)g0 * K, K, gsz, j, K, sl);
    __syncthreads();
    if (tid < 64) {
        if (tid < K) st_pub(fa.gpart + grp * 64 + tid, (f_sh[0][tid] + f_sh[1][tid]) + (f_sh[2][tid] + f_sh[3][tid]));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tid == 0) {
            __hip_atomic_store((gu32_t*)(fa.ctr + 1 + grp), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            f_tk = __hip_atomic_fetch_add((gu32_t*)fa.ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    if (f_tk != (unsigned)(ngrp - 1)) return;                     // not the launch's last group
    f_sh[sl][j] = fin_gather(fa.gpart, 64, ngrp, j, K, sl);
    __syncthreads();
    if (tid < 64) {
        f_tot[tid] = (f_sh[0][tid] + f_sh[1][tid]) + (f_sh[2][tid] + f_sh[3][tid]);
        if (tid == 0) __hip_atomic_store((gu32_t*)fa.ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (fa.kind == 1) bn_stats_math(f_tot, fa.n, fa.C, fa.o0, fa.o1, fa.o2, fa.o3, fa.o4);
    else bn_bwd_math(f_tot, fa.n, fa.C, fa.o0, fa.o1, fa.o2, fa.o3);
}
static_assert(NT / 64 == 4, "fin_reduce adds four slices");
// one partial value: plain store when the host finishes (the finish kernel runs behind a kernel boundary), published otherwise
__device__ __forceinline__ void st_part(double* p, double v, const FinArgs& fa) {
    if (fa.kind) st_pub(p, v);
    else *p = v;
}

// frequency index of the input tap (ConvGeom); false when the tap falls outside / between samples
__device__ __forceinline__ bool tap_fi(const ConvGeom& g, int fo, int kf, int& fi) {
    if (g.f_mode == 0) {
        fi = fo * g.sf - g.pf + kf;
    } else {
        const int num = fo + g.pf - kf;                 // sf is 1 or 2 in this model
        if (num < 0 || (num & (g.sf - 1)) != 0) return false;
        fi = num >> (g.sf - 1);
    }
    return fi >= 0 && fi < g.Fin;
}

// the same with the stride known to be 1 at compile time (the 3x3 and 1x1 layers): two adds and a range check instead
// of the run-time mode / stride / parity logic -- which cost ~50 scalar and vector instructions per tap of the MFMA
// conv kernels, issued between MFMAs that block the vector unit
template <bool SF1>      // SF1: stride 1; otherwise stride 2 (the 1x5 layers), branch free
__device__ __forceinline__ bool tap_fi_t(const ConvGeom& g, int fo, int kf, int& fi) {
    if constexpr (SF1) {
        fi = g.f_mode ? fo + g.pf - kf : fo - g.pf + kf;
        return fi >= 0 && fi < g.Fin;
    } else {
        const int n0 = fo * 2 - g.pf + kf, n1 = fo + g.pf - kf;
        fi = g.f_mode ? n1 >> 1 : n0;
        const bool par = g.f_mode ? (n1 >= 0 && (n1 & 1) == 0) : true;
        return par && fi >= 0 && fi < g.Fin;
    }
}

// ---- storage of the SAVED tensors (conv outputs y, activations a, block outputs: what the backward re-reads) -------
// fp32 (the reference's own precision) or bf16 (BASELINE configs[3]: half the bytes of every pass that touches them;
// arithmetic, statistics, gradients and master weights stay fp32).  The flag is a launch constant (wave-uniform
// branch in front of a memory access of a streaming kernel: free); a bf16 tensor is addressed through the same
// `float*` handle, its elements are 2 bytes wide.  Stores round to nearest even (v_cvt_pk_bf16_f32).
// format codes: 0 fp32, non-zero bf16.  (Rounds 2-4 also carried a saturating fp16 format, code 2, for the diagnostic storage
// modes that located the bf16 gradient noise.  With the format a RUN-TIME argument of most helpers below, every 16-bit
// conversion then computed BOTH encodings and selected one -- about 12 vector instructions per rounded element instead
// of 3 -- which is why k_dw16<3,1,PRE> took 165 us on bf16 tensors against 127 us on fp32 ones
// (profiles/r05_train_{f32,bf16}_kernel_stats.csv).  Round 5 removed the fp16 format: the diagnostics are answered,
// DESIGN.md section 8.)
__device__ __forceinline__ float bf2f(unsigned h) { return __uint_as_float(h << 16); }
__device__ __forceinline__ unsigned f2bf(float x) {
    const __bf16 h = (__bf16)x;
    return (unsigned)__builtin_bit_cast(unsigned short, h);
}
__device__ __forceinline__ float dec16(unsigned h, int fmt) { (void)fmt; return bf2f(h); }
__device__ __forceinline__ unsigned enc16(float x, int fmt) { (void)fmt; return f2bf(x); }
// two elements in ONE v_cvt_pk_bf16_f32 (a in the low half): the element-wise form above spends one conversion plus the
// masking / merging of its half on every element -- ~5 vector instructions per stored pair instead of 1
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned enc16x2(float a, float b) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2_t{a, b}, bf16x2_t));
}
// one element.  NOTE for callers with unrolled load loops (the weight-gradient kernels): make `fmt` a COMPILE-TIME
// constant there (template parameter).  A run-time `if (fmt)` around each load splits the loop into one basic block
// per load, so the 36 loads of an iteration are no longer issued together (measured 1.8x longer with bf16 storage
// than with fp32); a branch-free select form costs the fp32 path 10 % instead.
__device__ __forceinline__ float sld1(const float* base, long idx, int fmt) {
    return fmt ? dec16(reinterpret_cast<const unsigned short*>(base)[idx], fmt) : base[idx];
}
// Compile-time format, load and decode SEPARATED: sld1_raw returns the dword that holds the element (for a 16-bit
// format the aligned word, shifted so that the element sits in the low half), sld1_dec turns it into the value.
// Callers with predicated loads (`ok ? load : 0`) keep only the raw load under the predicate and decode after ALL
// loads of the iteration have been issued: decoding inside the predicated block puts an s_waitcnt vmcnt(0) behind
// every load (measured: the weight-gradient kernels 1.7x slower with bf16 storage than with fp32).
template <int FMT>
__device__ __forceinline__ unsigned sld1_raw(const float* base, long idx) {      // NOTHING here may use the loaded value
    if constexpr (FMT == 0) return __float_as_uint(base[idx]);
    else return reinterpret_cast<const unsigned*>(base)[idx >> 1];
}
template <int FMT>
__device__ __forceinline__ float sld1_dec(unsigned w, unsigned odd) {             // odd = idx & 1 of the element
    if constexpr (FMT == 0) return __uint_as_float(w);
    else return dec16((odd ? w >> 16 : w) & 0xFFFFu, FMT);
}
__device__ __forceinline__ void sst1(float* base, long idx, int fmt, float v) {
    if (fmt) reinterpret_cast<unsigned short*>(base)[idx] = (unsigned short)enc16(v, fmt);
    else base[idx] = v;
}
// NTL: nontemporal load, for the passes that read every element exactly once.  A tensor the PREVIOUS kernel has just
// written (every gradient, every conv output) is still dirty in the Infinity Cache; a plain streaming read of two
// 271 MB tensors, one of them just written, runs at 4.65 TB/s, the same read with nontemporal loads at 6.68 TB/s
// (tools/ubench_reduce_bw.hip: without the preceding writer 6.24 against 6.53)
// Same-box A/Bs of the fp32 step (tools/ab_bench.py style, GTCRN_LIB_VARIANT=exp): nontemporal loads in the read-once
// passes 46.2-47.0 ms against 47.9-48.7 with plain loads; the same hint on loads that are re-read by neighbouring taps
// (k_dw16, the 3x3 / 1x5 convs and weight gradients) 48.3 against 46.8 -- worse, not used; on the conv / weight-gradient
// operands that are read once 45.8 against 45.9 -- nothing; nontemporal STORES of the streamed outputs 46.2 against 46.5.
constexpr bool kNt = true;      // loads of the read-once passes
constexpr bool kNtSt = true;    // stores of tensors a later kernel streams through once
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
template <bool NTL = false>
__device__ __forceinline__ f32x4 sld4(const float* base, long idx, int fmt) {      // idx % 4 == 0
    if (fmt) {
        const u32x2* p = reinterpret_cast<const u32x2*>(reinterpret_cast<const unsigned short*>(base) + idx);
        const u32x2 u = NTL ? __builtin_nontemporal_load(p) : *p;
        return f32x4{dec16(u.x & 0xFFFFu, fmt), dec16(u.x >> 16, fmt), dec16(u.y & 0xFFFFu, fmt), dec16(u.y >> 16, fmt)};
    }
    const f32x4* p = reinterpret_cast<const f32x4*>(base + idx);
    return NTL ? __builtin_nontemporal_load(p) : *p;
}
template <bool NTS = false>
__device__ __forceinline__ void sst4(float* base, long idx, int fmt, const f32x4 v) {
    if (fmt) {
        u32x2 u;
        u.x = enc16x2(v[0], v[1]);
        u.y = enc16x2(v[2], v[3]);
        u32x2* p = reinterpret_cast<u32x2*>(reinterpret_cast<unsigned short*>(base) + idx);
        if (NTS) __builtin_nontemporal_store(u, p); else *p = u;
    } else {
        f32x4* p = reinterpret_cast<f32x4*>(base + idx);
        if (NTS) __builtin_nontemporal_store(v, p); else *p = v;
    }
}
__device__ __forceinline__ float round16(float x, int fmt) { return fmt ? dec16(enc16(x, fmt), fmt) : x; }
__device__ __forceinline__ f32x4 round_bf4(const f32x4 v, int fmt) {
    if (!fmt) return v;
    const unsigned a = enc16x2(v[0], v[1]), b = enc16x2(v[2], v[3]);       // (same round-to-nearest-even as enc16)
    return f32x4{__uint_as_float(a << 16), __uint_as_float(a & 0xFFFF0000u), __uint_as_float(b << 16), __uint_as_float(b & 0xFFFF0000u)};
}
template <int C, bool NTL = false>
__device__ __forceinline__ void load_vec_s(const float* base, long idx, int bf, float (&v)[C]) {
    if constexpr (C % 4 == 0) {
#pragma unroll
        for (int i = 0; i < C; i += 4) {
            const f32x4 t = sld4<NTL>(base, idx + i, bf);
            v[i] = t[0]; v[i + 1] = t[1]; v[i + 2] = t[2]; v[i + 3] = t[3];
        }
    } else {
#pragma unroll
        for (int i = 0; i < C; ++i) v[i] = sld1(base, idx + i, bf);
    }
}

template <int C, bool NTL = false>
__device__ __forceinline__ void load_vec(const float* p, float (&v)[C]) {
    if constexpr (C % 4 == 0) {
#pragma unroll
        for (int i = 0; i < C; i += 4) {
            const f32x4 t = NTL ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + i))
                                : *reinterpret_cast<const f32x4*>(p + i);
            v[i] = t[0]; v[i + 1] = t[1]; v[i + 2] = t[2]; v[i + 3] = t[3];
        }
    } else {
#pragma unroll
        for (int i = 0; i < C; ++i) v[i] = p[i];
    }
}

// ------------------------------------------------------------------------------ dense conv
// nn.Conv2d / nn.ConvTranspose2d of ConvBlock (models/gtcrn_micro.py:142-164), GTConvBlock
// (:167-253) and TCN conv1/conv3 (:268-287), and their data gradients.
template <int CIN, int COUT>
// shift (bf16 output only): the tensor is stored as y - shift[c].  A train-mode BatchNorm follows and is invariant to
// a per-channel shift; with shift = the channel's batch mean of the PREVIOUS step (k_bn_stats_finish maintains it;
// the running mean before the first step) the stored values are centred, so their bf16 rounding error is relative to
// the channel's SPREAD, not to its offset (|mean| >> std would otherwise be amplified by |mean| / std after
// normalisation).
__global__ __launch_bounds__(NT) void k_conv(ConvGeom g, const float* __restrict__ in, const float* __restrict__ w,
                                            const float* __restrict__ bias, float* __restrict__ out,
                                            const float* __restrict__ shift) {
    __shared__ __attribute__((aligned(16))) float sW[9 * CIN * COUT];   // [tap][ci][co]
    const int tid = threadIdx.x, ntap = g.nkt * g.nkf;
    for (int i = tid; i < ntap * CIN * COUT; i += NT) {
        const int tap = i / (CIN * COUT), r = i - tap * (CIN * COUT), ci = r / COUT, co = r - ci * COUT;
        const int kt = tap / g.nkf, kf = tap - kt * g.nkf;
        sW[i] = w[co * g.w_co + ci * g.w_ci + kt * g.w_kt + kf * g.w_kf];
    }
    __syncthreads();
    const long npos = (long)g.B * g.Tout * g.Fout;
    // (positions fit in 31 bits -- the launcher checks: 32-bit divisions; the 64-bit ones by the run-time Fout / Tout were a
    // third of this kernel's instructions)
    const unsigned uF = (unsigned)g.Fout, uT = (unsigned)g.Tout;
    for (long p = (long)blockIdx.x * NT + tid; p < npos; p += (long)gridDim.x * NT) {
        const unsigned pu = (unsigned)p, ubt = pu / uF, ub = ubt / uT;
        const int fo = (int)(pu - ubt * uF);
        const int to = (int)(ubt - ub * uT), b = (int)ub;
        float acc[COUT];
#pragma unroll
        for (int co = 0; co < COUT; ++co) acc[co] = (bias ? bias[co] : 0.f) - (shift ? shift[co] : 0.f);
        for (int kt = 0; kt < g.nkt; ++kt) {
            const int ti = to + g.t_off[kt];
            if (ti < 0 || ti >= g.Tin) continue;
            for (int kf = 0; kf < g.nkf; ++kf) {
                int fi;
                if (!tap_fi(g, fo, kf, fi)) continue;
                float xv[CIN];
                load_vec_s<CIN>(in, (((long)b * g.Tin + ti) * g.Fin + fi) * g.CinT + g.cin_off, g.in_bf, xv);
                const float* wt = sW + (kt * g.nkf + kf) * CIN * COUT;
#pragma unroll
                for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
                    for (int co = 0; co < COUT; ++co) acc[co] = fmaf(wt[ci * COUT + co], xv[ci], acc[co]);
            }
        }
        if (g.out_bf) {
#pragma unroll
            for (int co = 0; co < COUT; ++co) sst1(out, p * g.CoutT + g.cout_off + co, g.out_bf, acc[co]);
        } else {
            float* o = out + p * g.CoutT + g.cout_off;
#pragma unroll
            for (int co = 0; co < COUT; ++co) o[co] = g.accumulate ? o[co] + acc[co] : acc[co];
        }
    }
}


// sum of a double over the lanes of a wave whose lane numbers differ only in the bits LO..HI (powers of two, as xor
// distances), largest distance first: a fixed order, every lane ends with the same total
__device__ __forceinline__ double wave_sum_xor(double s, int lo, int hi) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        if (off <= hi && off >= lo) s += __shfl_xor(s, off, 64);
    return s;
}
// sequential sum of p[w * K] for w = w0, w0 + step, ... < n, the loads issued eight at a time (one at a time every
// load of these small second-stage reductions paid its own L2/MALL round trip: ~19 us per launch, 130 launches a step)
template <class T>
__device__ __forceinline__ double sum_strided(const T* __restrict__ p, int w0, int n, int step, long K) {
    double s = 0.0;
    int w = w0;
    for (; w + 7 * step < n; w += 8 * step) {
        T t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = p[(long)(w + u * step) * K];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += (double)t[u];
    }
    for (; w < n; w += step) s += (double)p[(long)w * K];
    return s;
}

// ------------------------------------------------------------------ dense conv on the matrix cores
// Same arithmetic as k_conv / k_conv_wgrad for channel counts that are multiples of 4 (all the
// 16/8-channel layers), on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation):
//   forward / data gradient: a tile = 16 consecutive output positions; lane (n = lane&15, g = lane>>4)
//     loads the 4 input channels 4g..4g+3 of position n for each tap (one coalesced 16-byte load), the
//     weights sit in LDS as 16x16 matrices [tap][co][ci] read as A fragments; the D fragment is
//     channels 4g..4g+3 of position n again: one 16-byte store per lane.
//   weight gradient: the contraction runs over positions, so positions are the K index: lane (c, k)
//     loads channel c of position 4*group + k of dout (A) and of the tap-shifted input (B); one MFMA per
//     tap per 4 positions accumulates the full 16x16 dW of that tap in registers.
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// (b, t, f) of a flat position, advanced incrementally (rows have >= 16 positions)
struct Pos {
    int f, t, b;
    __device__ __forceinline__ void init(long p, int F, int T) {
        f = (int)(p % F);
        const long bt = p / F;
        t = (int)(bt % T);
        b = (int)(bt / T);
    }
    __device__ __forceinline__ void advance(int step, int F, int T) {
        f += step;
        if (f >= F) { f -= F; if (++t >= T) { t = 0; ++b; } }
    }
};

// Position of a grid-stride loop over flat positions, advanced by a launch-constant stride without divisions:
// stride = a * F + r positions, a = a1 * T + a0 rows (r, a, a0 are computed on the host).
struct StrideIter {
    int r, a, a0;
};
inline StrideIter stride_iter(long stride_pos, int F, int T) {
    StrideIter s;
    s.r = (int)(stride_pos % F);
    s.a = (int)(stride_pos / F);
    s.a0 = s.a % T;
    return s;
}
struct RowPos {
    int fo, to, bt;       // bin, frame inside the utterance, flat row b*T + t
    __device__ __forceinline__ void init(long p, int F, int T) {
        fo = (int)(p % F);
        bt = (int)(p / F);
        to = bt % T;
    }
    __device__ __forceinline__ void advance(const StrideIter& s, int F, int T) {
        fo += s.r;
        int carry = 0;
        if (fo >= F) { fo -= F; carry = 1; }
        bt += s.a + carry;
        to += s.a0 + carry;
        if (to >= T) to -= T;
        if (to >= T) to -= T;
    }
};

// 16-byte (4-channel) operand loads with the storage format as a compile-time constant, load and decode separated
template <int FMT> struct Raw4 { using t = f32x4; };
template <> struct Raw4<1> { using t = uint2; };
template <> struct Raw4<2> { using t = uint2; };
template <int FMT, bool NTL = false>
__device__ __forceinline__ typename Raw4<FMT>::t sld4_raw(const float* base, long idx) {      // idx % 4 == 0
    if constexpr (FMT == 0) {
        const f32x4* p = reinterpret_cast<const f32x4*>(base + idx);
        return NTL ? __builtin_nontemporal_load(p) : *p;
    } else {
        const u32x2* p = reinterpret_cast<const u32x2*>(reinterpret_cast<const unsigned short*>(base) + idx);
        const u32x2 u = NTL ? __builtin_nontemporal_load(p) : *p;
        return uint2{u.x, u.y};
    }
}
template <int FMT>
__device__ __forceinline__ f32x4 dec4(const typename Raw4<FMT>::t r) {
    if constexpr (FMT == 0) return r;
    else return f32x4{dec16(r.x & 0xFFFFu, FMT), dec16(r.x >> 16, FMT), dec16(r.y & 0xFFFFu, FMT), dec16(r.y >> 16, FMT)};
}
// BnPre (train_kernels.h): the previous unit's BatchNorm + PReLU applied to a loaded quad of its conv output -- the
// expressions of k_bn_act, so the values are bit-identical to the separate pass -- rounded to the activation's storage
// format (what a later reader of the stored activation would see)
struct PreConst {
    f32x4 mean, istd, gm, bt;
    float sl;
    bool act;
};
__device__ __forceinline__ PreConst pre_const(const BnPre& pre, int q, int C) {
    PreConst k;
    k.mean = *reinterpret_cast<const f32x4*>(pre.stats + 4 * q);
    k.istd = *reinterpret_cast<const f32x4*>(pre.stats + C + 4 * q);
    k.gm = *reinterpret_cast<const f32x4*>(pre.gamma + 4 * q);
    k.bt = *reinterpret_cast<const f32x4*>(pre.beta + 4 * q);
    k.act = pre.slope != nullptr;
    k.sl = k.act ? pre.slope[0] : 0.f;
    return k;
}
// Exact chain: the 16-bit copy of a conv output y that the BACKWARD re-reads, written by y's consumer (which knows this
// step's statistics): yt = bf16(y - mean), i.e. centred exactly (the backward's statistics for it are mean 0, invstd),
// and -- the part that matters -- on the SAME side of the PReLU kink as the forward's z: the backward recomputes
// z = gamma * (yt * invstd) + beta [+ bf16(res)] from the copy, and where plain rounding would move it across zero
// (a fraction ~1e-3 of the elements of a layer, each then wrong by (1 - slope) * da: 2-3 % of the layer's gradient in
// relative L2, ~5 % over the depth of the network -- measured) the neighbouring bf16 value is stored instead.
__device__ __forceinline__ float bf16_step(float v, bool up) {       // next bf16 value above / below v (v is a bf16 value)
    unsigned u = __float_as_uint(v);
    if ((u << 1) == 0) return __uint_as_float(up ? 0x00010000u : 0x80010000u);
    const bool neg = (u >> 31) != 0;
    u = (up != neg) ? u + 0x10000u : u - 0x10000u;
    return __uint_as_float(u);
}
__device__ __forceinline__ float ycopy_value(float y, float z, float mean, float istd, float gm, float bt, bool has_res,
                                             float res, int bf, bool kink) {
    float yt = round16(y - mean, bf);
    if (kink && bf == 1) {
        const float rt = has_res ? round16(res, bf) : 0.f;            // what the backward will load as the residual
        auto zb = [&](float v) { float q = gm * ((v - 0.f) * istd) + bt; if (has_res) q += rt; return q; };
        if ((zb(yt) > 0.f) != (z > 0.f)) {
            const float up = bf16_step(yt, true), dn = bf16_step(yt, false);
            if ((zb(up) > 0.f) == (z > 0.f)) yt = up;
            else if ((zb(dn) > 0.f) == (z > 0.f)) yt = dn;
        }
    }
    return yt;
}
// the previous unit's activation, handed on by a normalise-on-load conv: rounded 16-bit copy for the backward (always),
// and in the exact-chain mode the fp32 value for the activation's other readers
__device__ __forceinline__ void pre_store(const BnPre& pre, long idx, const f32x4 a) {
    if (pre.a_out) sst4<kNtSt>(pre.a_out, idx, pre.bf, a);      // (nullptr: the backward recomputes it from y, see NextRedArgs)
    if (pre.exact && pre.a_chain) sst4<kNtSt>(pre.a_chain, idx, 0, a);
}
// ... and, exact chain, the centred copy of the previous unit's conv output y (see ycopy_value)
__device__ __forceinline__ void pre_store_y(const BnPre& pre, const PreConst& k, long idx, const f32x4 y, bool has_res,
                                            const f32x4 r) {
    if (!pre.exact || !pre.y_out) return;
    f32x4 t;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float z = k.gm[e] * ((y[e] - k.mean[e]) * k.istd[e]) + k.bt[e];
        if (has_res) z += r[e];
        t[e] = ycopy_value(y[e], z, k.mean[e], k.istd[e], k.gm[e], k.bt[e], has_res, r[e], pre.ybf_out, k.act);
    }
    sst4<kNtSt>(pre.y_out, idx, pre.ybf_out, t);
}
__device__ __forceinline__ f32x4 pre_apply(const PreConst& k, const f32x4 y, int bf, bool has_res = false,
                                           const f32x4 r = f32x4{0.f, 0.f, 0.f, 0.f}) {
    f32x4 a;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float z = k.gm[e] * ((y[e] - k.mean[e]) * k.istd[e]) + k.bt[e];
        if (has_res) z += r[e];
        a[e] = k.act ? (z > 0.f ? z : k.sl * z) : z;
    }
    return round_bf4(a, bf);
}

// four consecutive elements starting at ANY element index (4-byte / 2-byte aligned): one global_load_dwordx4 /
// dwordx2 (the hardware takes unaligned vector loads; gfx950 runs in unaligned access mode under ROCm)
template <int FMT>
__device__ __forceinline__ typename Raw4<FMT>::t sldw_raw(const float* base, long idx) {
    if constexpr (FMT == 0) {
        typedef f32x4 f32x4u __attribute__((aligned(4)));
        return *reinterpret_cast<const f32x4u*>(base + idx);
    } else {
        typedef u32x2 u32x2u __attribute__((aligned(2)));
        const u32x2u u = *reinterpret_cast<const u32x2u*>(reinterpret_cast<const unsigned short*>(base) + idx);
        return uint2{u.x, u.y};
    }
}
// The two narrow layers (encoder.en_convs.0: 3 -> 16 channels, decoder.de_convs.4: 16 -> 2, both (1,5) stride 2) as
// WINDOW products.  The taps of one 16-channel position p = (row, f) are nkf * Cn CONSECUTIVE elements of the narrow
// tensor's row, starting at element (sf * f - pf) * Cn: j = kf * Cn + c.  So with the weights as one 16 x 16 matrix
// [wide channel][j] the conv / its adjoint is ONE K = 16 MFMA chain per 16 positions whose B operand is the window
// (lane (n, q) loads elements 4q..4q+3 of position n's window: one unaligned 16-byte load), and the weight gradient
// is one MFMA per four positions -- instead of five taps with 3 (2) live channels of 16 each, fed by 4-byte loads.
// (A row of the narrow tensor has sf * (Fw - 1) + 1 bins, so the windows of a tile that runs over the end of a row
// simply continue into the next one; elements outside the own row are masked.)
struct WinPos {
    long idx;        // flat element index of the lane's first window element
    bool ok[4];
    bool any, edge;
};
__device__ __forceinline__ WinPos win_pos(const Pos& P, bool pv, int q, int Cn, int J, int sf, int pf, int T, long rowlen,
                                          long total) {
    WinPos w;
    const int e0 = (P.f * sf - pf) * Cn + 4 * q;          // relative to the row
    w.idx = ((long)P.b * T + P.t) * rowlen + e0;
    w.any = false;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        w.ok[s] = pv && 4 * q + s < J && e0 + s >= 0 && e0 + s < rowlen;
        w.any = w.any || w.ok[s];
    }
    w.edge = w.idx < 0 || w.idx + 4 > total;               // the vector would leave the tensor: element-wise loads
    return w;
}
template <int FMT>
__device__ __forceinline__ f32x4 win_value(const float* base, const WinPos& w, const typename Raw4<FMT>::t raw) {
    const f32x4 d = dec4<FMT>(raw);
    f32x4 x;
#pragma unroll
    for (int s = 0; s < 4; ++s) x[s] = w.ok[s] ? d[s] : 0.f;
    if (w.any && w.edge) {                                 // first / last position of the whole tensor only
#pragma unroll
        for (int s = 0; s < 4; ++s) x[s] = w.ok[s] ? sld1(base, w.idx + s, FMT) : 0.f;
    }
    return x;
}
// the unit whose gradient input is the dx a backward kernel produces (16 channels, PReLU; res: its residual input or
// nullptr): that unit's first backward pass -- sum dz, sum dz * xhat, sum of the slope terms -- is accumulated by the
// producing kernel from one more read of its y (and res) instead of a pass that re-reads dx as well
// XR (with NEXT): that unit's activation is this unit's input x, and it is not read but RECOMPUTED from the y (and res)
// loaded for the reduction -- one tensor read less, and the forward need not store the activation at all when this
// backward is its only other reader.  xround: the forward's consumer convolved the activation rounded to the 16-bit
// storage format (bf16 storage; not the exact chain), so the recomputed one is rounded the same way.
struct NextRedArgs {
    const float *y, *stats, *gamma, *beta, *slope, *res;
    int xround;
    int yfmt;      // storage format of y (the kernels that do not take it as a template parameter: conv / depthwise adjoints)
};
// ... the same riding reduction in the epilogue of a conv that produces that gradient input as its OUTPUT (the adjoint
// conv of a depthwise / dense 3x3 unit, of en_convs.1): constants of the lane's channel quad, and the three sums
struct NextConst {
    f32x4 mean, istd, gm, bt;
    float sl;
};
__device__ __forceinline__ NextConst next_const(const NextRedArgs& nx, int q4) {
    NextConst k;
    k.mean = *reinterpret_cast<const f32x4*>(nx.stats + q4); k.istd = *reinterpret_cast<const f32x4*>(nx.stats + 16 + q4);
    k.gm = *reinterpret_cast<const f32x4*>(nx.gamma + q4); k.bt = *reinterpret_cast<const f32x4*>(nx.beta + q4);
    k.sl = nx.slope[0];
    return k;
}
// that unit's activation PReLU(BatchNorm(y)) as pre_apply / k_bn_act form it (xround: rounded to bf16 like the stored one)
__device__ __forceinline__ f32x4 next_act(const NextConst& k, const f32x4 y, int xround) {
    f32x4 a;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float z = k.gm[e] * ((y[e] - k.mean[e]) * k.istd[e]) + k.bt[e];
        a[e] = z > 0.f ? z : k.sl * z;
    }
    // (a select per element, not a branch around the rounding: the branch cost k_dense33_bwd's fp32 form 30 registers)
    const f32x4 r = round_bf4(a, 1);
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = xround ? r[e] : a[e];
    return a;
}
__device__ __forceinline__ void next_accum(const NextConst& k, const f32x4 y, const f32x4 g, float (&vr)[3][4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float xh = (y[e] - k.mean[e]) * k.istd[e];
        const float z = k.gm[e] * xh + k.bt[e];
        const float dz = z > 0.f ? g[e] : k.sl * g[e];          // act_bwd, PReLU
        vr[0][e] += dz;
        vr[1][e] = fmaf(dz, xh, vr[1][e]);
        vr[2][e] += z > 0.f ? 0.f : g[e] * z;
    }
}
// FIN: storage format of `in` (compile time).  All tap loads of a tile are issued before the first MFMA: a tap outside
// the tensor loads element 0 and is zeroed by a select -- with `if (ok) load` every tap sat in its own basic block and
// the tile paid nine L2 latencies one after the other (the 3x3 convs ran at 45 TFLOP/s, latency-bound).
// WIN: the window form above (NKT = NKF = 1 then: one 16 x 16 matrix [co][j])
// PRE: 1x1 only; `in` is the previous unit's conv output, see BnPre
// NEXT: the output IS the gradient input of a 16-channel PReLU unit (see NextRedArgs): its reduction rides in the epilogue,
// per-workgroup sums [48] into stat_partial (which the forward's statistics do not use in a backward launch)
template <int NKT, int NKF, int FIN, bool WIN = false, bool PRE = false, int NEXT = 0>   // NEXT: 1 + storage format of that y
__global__ __launch_bounds__(NT) void k_conv_mfma(ConvGeom g, const float* __restrict__ in,
                                                 const float* __restrict__ w, const float* __restrict__ bias,
                                                 float* __restrict__ out, long tiles_per_wave,
                                                 double* __restrict__ stat_partial, const float* __restrict__ shift,
                                                 BnPre pre, NextRedArgs nx, FinArgs fa) {
    static_assert(!PRE || (NKT * NKF == 1 && !WIN), "normalise-on-load: pointwise convs only");
    static_assert(!NEXT || (!PRE && !WIN), "riding reduction: plain adjoint launches");
    NextConst nk{};
    float vr[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) vr[0][e] = vr[1][e] = vr[2][e] = 0.f;
    if constexpr (NEXT) nk = next_const(nx, 4 * ((threadIdx.x & 63) >> 4));
    __shared__ __attribute__((aligned(16))) float sW[NKT * NKF * 256];   // [tap][co][ci], zero padded
    __shared__ double sStat[NT / 64][32];   // per wave: sum[16], sum of squares[16]
    const int tid = threadIdx.x;
    for (int i = tid; i < NKT * NKF * 256; i += NT) {
        const int tap = i >> 8, co = (i >> 4) & 15, ci = i & 15, kt = tap / NKF, kf = tap - kt * NKF;
        if constexpr (WIN) {
            const int wk = ci / g.Cin, wc = ci - wk * g.Cin;        // j = ci: tap wk, channel wc
            sW[i] = (co < g.Cout && wk < g.nkf) ? w[co * g.w_co + wc * g.w_ci + wk * g.w_kf] : 0.f;
        } else {
            sW[i] = (co < g.Cout && ci < g.Cin) ? w[co * g.w_co + ci * g.w_ci + kt * g.w_kt + kf * g.w_kf] : 0.f;
        }
    }
    __syncthreads();
    const int lane = tid & 63, n = lane & 15, q = lane >> 4;
    const long npos = (long)g.B * g.Tout * g.Fout, ntiles = (npos + 15) >> 4;
    const long wave = (long)blockIdx.x * (NT / 64) + (tid >> 6);
    long tile = wave * tiles_per_wave;
    const long tend = tile + tiles_per_wave < ntiles ? tile + tiles_per_wave : ntiles;
    // BatchNorm statistics of this lane's outputs, accumulated in DOUBLE from the first addition on (the squares are
    // exact products of two floats): var = E[y^2] - mean^2 then survives |mean| >> std (a large conv bias, a
    // near-constant channel), where fp32 per-thread sums lose the variance's leading digits
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    Pos P;
    {
        const long p0 = tile * 16 + n;
        P.init(p0 < npos ? p0 : npos - 1, g.Fout, g.Tout);
    }
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (bias && 4 * q < g.Cout) bv = *reinterpret_cast<const f32x4*>(bias + 4 * q);
    if (shift && 4 * q < g.Cout) bv -= *reinterpret_cast<const f32x4*>(shift + 4 * q);
    const bool cin_ok = 4 * q < g.Cin, cout_ok = 4 * q < g.Cout;
    PreConst pk{};
    if constexpr (PRE) pk = pre_const(pre, q, g.CinT);
    if constexpr (NKT * NKF == 1 && !WIN && !NEXT && FIN != 0) {
        // Pointwise convs (28 launches of a step, 21 of them normalise-on-load): SOFTWARE-PIPELINED over the wave's tiles --
        // the loads of tile i + 1 (its 16 bytes per lane of input, and of the residual) are in flight while tile i is
        // normalised, multiplied and stored.  With one tile's loads per wave at a time the kernel had 20 KB in flight per
        // CU (five waves per SIMD x 1 KB) against the ~47 KB that 6 TB/s x the memory latency asks for: it moved 3.6 TB/s
        // in fp32 storage and took the SAME time on half the bytes in bf16 storage (profiles/r05_train_*_kernel_stats.csv).
        // Same expressions in the same order per tile: bit-identical results.
        struct TileIn {
            typename Raw4<FIN>::t raw;
            f32x4 pres;
            long pidx;
            bool ok;
        };
        auto fetch = [&](const Pos& Q, bool pv_, TileIn& ti_) {
            const int ti = Q.t + g.t_off[0];
            const bool okt = pv_ && cin_ok && ti >= 0 && ti < g.Tin;
            const long rowbase = ((long)Q.b * g.Tin + ti) * g.Fin;
            int fi;
            ti_.ok = tap_fi_t<true>(g, Q.f, 0, fi) && okt;
            ti_.pidx = (rowbase + fi) * g.CinT + g.cin_off + 4 * q;
            ti_.raw = sld4_raw<FIN>(in, ti_.ok ? ti_.pidx : 0L);
            ti_.pres = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (PRE)
                if (pre.res) ti_.pres = sld4(pre.res, ti_.ok ? ti_.pidx : 0L, pre.exact ? 0 : pre.bf);
        };
        TileIn cur, nxt;
        if (tile < tend) fetch(P, tile * 16 + n < npos, cur);
        for (; tile < tend; ++tile) {
            const long p = tile * 16 + n;
            const bool pv = p < npos;
            Pos Pn = P;
            Pn.advance(16, g.Fout, g.Tout);
            nxt = cur;
            if (tile + 1 < tend) fetch(Pn, p + 16 < npos, nxt);          // (wave-uniform branch)
            f32x4 acc = bv;
            f32x4 d = dec4<FIN>(cur.raw);
            if constexpr (PRE) {
                const f32x4 yraw = d;
                d = pre_apply(pk, d, pre.exact ? 0 : pre.bf, pre.res != nullptr, cur.pres);
                if (cur.ok) {
                    pre_store(pre, cur.pidx, d);
                    pre_store_y(pre, pk, cur.pidx, yraw, pre.res != nullptr, cur.pres);
                }
            }
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            const f32x4 xv = cur.ok ? d : zero;
            const f32x4 A = *reinterpret_cast<const f32x4*>(sW + n * 16 + 4 * q);
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) acc = mfma4(A[s4], xv[s4], acc);
            if (pv && cout_ok) {
                if (g.out_bf) {
                    acc = round_bf4(acc, g.out_bf);
                    sst4<kNtSt>(out, p * g.CoutT + g.cout_off + 4 * q, g.out_bf, acc);
                } else {
                    f32x4* o = reinterpret_cast<f32x4*>(out + p * g.CoutT + g.cout_off + 4 * q);
                    if (g.accumulate) { acc = *o + acc; *o = acc; }
                    else sst4<kNtSt>(out, p * g.CoutT + g.cout_off + 4 * q, 0, acc);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) { const double a = (double)acc[e]; s1[e] += a; s2[e] = fma(a, a, s2[e]); }
            }
            cur = nxt;
            P = Pn;
        }
    } else
    for (; tile < tend; ++tile) {
        const long p = tile * 16 + n;
        const bool pv = p < npos;
        f32x4 acc = bv;
        f32x4 ynx = {0.f, 0.f, 0.f, 0.f};
        if constexpr (NEXT) ynx = dec4<NEXT ? NEXT - 1 : 0>(sld4_raw<NEXT ? NEXT - 1 : 0, true>(nx.y, (pv ? p : 0) * 16 + 4 * q));   // (CoutT == 16: the launcher checks)
        if constexpr (WIN) {
            const long rowlen = (long)g.Fin * g.Cin;
            const WinPos wp = win_pos(P, pv, q, g.Cin, g.Cin * g.nkf, g.sf, g.pf, g.Tin, rowlen, (long)g.B * g.Tin * rowlen);
            const typename Raw4<FIN>::t raw = sldw_raw<FIN>(in, (wp.any && !wp.edge) ? wp.idx : 0L);
            const f32x4 xv = win_value<FIN>(in, wp, raw);
            const f32x4 A = *reinterpret_cast<const f32x4*>(sW + n * 16 + 4 * q);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = mfma4(A[s], xv[s], acc);
        } else {
        typename Raw4<FIN>::t raw[NKT * NKF];
        bool okv[NKT * NKF];
        long pidx = 0;
        f32x4 pres = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            const int ti = P.t + g.t_off[kt];
            const bool okt = pv && cin_ok && ti >= 0 && ti < g.Tin;
            const long rowbase = ((long)P.b * g.Tin + ti) * g.Fin;
#pragma unroll
            for (int kf = 0; kf < NKF; ++kf) {
                int fi;
                const bool ok = tap_fi_t<NKF != 5>(g, P.f, kf, fi) && okt;      // (only the 1x5 layers are strided)
                okv[kt * NKF + kf] = ok;
                raw[kt * NKF + kf] = sld4_raw<FIN>(in, ok ? (rowbase + fi) * g.CinT + g.cin_off + 4 * q : 0L);
                if constexpr (PRE) {
                    pidx = (rowbase + fi) * g.CinT + g.cin_off + 4 * q;
                    if (pre.res) pres = sld4(pre.res, ok ? pidx : 0L, pre.exact ? 0 : pre.bf);
                }
            }
        }
#pragma unroll
        for (int tap = 0; tap < NKT * NKF; ++tap) {
            f32x4 d = dec4<FIN>(raw[tap]);
            if constexpr (PRE) {
                const f32x4 yraw = d;
                d = pre_apply(pk, d, pre.exact ? 0 : pre.bf, pre.res != nullptr, pres);
                if (okv[tap]) {
                    pre_store(pre, pidx, d);
                    pre_store_y(pre, pk, pidx, yraw, pre.res != nullptr, pres);
                }
            }
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            const f32x4 xv = okv[tap] ? d : zero;
            const f32x4 A = *reinterpret_cast<const f32x4*>(sW + tap * 256 + n * 16 + 4 * q);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = mfma4(A[s], xv[s], acc);
        }
        }
        if (pv && cout_ok) {
            if (g.out_bf) {
                // (accumulate with a 16-bit output: the adjoint convs of storage mode 5, whose dx is a bf16 gradient tensor)
                if (g.accumulate) acc = sld4(out, p * g.CoutT + g.cout_off + 4 * q, g.out_bf) + acc;
                acc = round_bf4(acc, g.out_bf);   // the statistics are those of the STORED tensor (the backward re-reads it)
                sst4<kNtSt>(out, p * g.CoutT + g.cout_off + 4 * q, g.out_bf, acc);
            } else {
                f32x4* o = reinterpret_cast<f32x4*>(out + p * g.CoutT + g.cout_off + 4 * q);
                if (g.accumulate) { acc = *o + acc; *o = acc; }
                else sst4<kNtSt>(out, p * g.CoutT + g.cout_off + 4 * q, 0, acc);
            }
            if constexpr (NEXT) next_accum(nk, ynx, acc, vr);          // (acc: the value the tensor now holds)
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) { const double a = (double)acc[e]; s1[e] += a; s2[e] = fma(a, a, s2[e]); }
            }
        }
        P.advance(16, g.Fout, g.Tout);
    }
    if constexpr (NEXT) {
        __shared__ double sRed[NT / 64][48];
#pragma unroll
        for (int k3 = 0; k3 < 3; ++k3)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double t = wave_sum_xor((double)vr[k3][e], 1, 8);
                if (n == 0) sRed[tid >> 6][k3 * 16 + 4 * q + e] = t;
            }
        __syncthreads();
        if (tid < 48) {
            double t = 0.0;
            for (int w2 = 0; w2 < NT / 64; ++w2) t += sRed[w2][tid];
            st_part(stat_partial + (long)blockIdx.x * 48 + tid, t, fa);
        }
        if (fa.kind) fin_reduce(stat_partial, 48, blockIdx.x, gridDim.x, fa);
        return;
    }
    if (stat_partial) {
        // per-workgroup sums of y and y^2 per channel (the conv is followed by a train-mode BatchNorm):
        // lanes -> LDS -> one thread per (sum, channel), fixed order; combined across workgroups by k_bn_stats_finish
        // (lanes of one channel quad differ in n = lane & 15: xor distances 8..1)
#pragma unroll
        for (int e = 0; e < 4; ++e) { s1[e] = wave_sum_xor(s1[e], 1, 8); s2[e] = wave_sum_xor(s2[e], 1, 8); }
        if (n == 0)
#pragma unroll
            for (int e = 0; e < 4; ++e) { sStat[tid >> 6][4 * q + e] = s1[e]; sStat[tid >> 6][16 + 4 * q + e] = s2[e]; }
        __syncthreads();
        if (tid < 2 * g.Cout) {
            const int which = tid / g.Cout, ch = tid - which * g.Cout;
            double t = 0.0;
            for (int w = 0; w < NT / 64; ++w) t += sStat[w][which * 16 + ch];
            st_part(stat_partial + (long)blockIdx.x * 2 * g.Cout + tid, t, fa);
        }
        if (fa.kind) fin_reduce(stat_partial, 2 * g.Cout, blockIdx.x, gridDim.x, fa);
    }
}

// ------------------------------------------------------------ the pointwise (1x1) forward convs, dedicated form
// 28 launches of a step (21 of them normalise-on-load) ran through k_conv_mfma<1, 1>, whose loop carries everything a
// strided, padded, multi-tap conv needs -- a (b, t, f) position per tile, 64-bit row arithmetic per tap, run-time format /
// residual / accumulate switches: ~250 vector instructions per 16-position tile, which is what bounded it (114 us on
// 272 MB of bf16 tensors, 148 us on 544 MB of fp32 ones: the same 4 waves per SIMD issue-bound either way).  A pointwise
// conv needs none of that: position p reads element p * CinT + cin_off and writes element p * Cout; per tile the lane
// advances two 32-bit offsets.  Formats, residual and normalise-on-load are compile-time; the A fragment of the one 16 x 16
// weight matrix stays in registers.  Same expressions in the same order as k_conv_mfma (pre_apply, bias first, four
// k-ordered MFMAs, statistics in double from the value the tensor holds): bit-identical outputs and statistics.
// (exact-chain storage and accumulating launches keep the general kernel.)
constexpr int PW_U = 2;
template <int FIN, int OUTF, bool PRE, bool RES>
__global__ __launch_bounds__(NT) void k_pw_fwd(long npos, int Cin, int CinT, int cin_off, int Cout, int w_co, int w_ci,
                                              const float* __restrict__ in, const float* __restrict__ w,
                                              const float* __restrict__ bias, float* __restrict__ out, long tiles_per_wave,
                                              double* __restrict__ stat_partial, const float* __restrict__ shift, BnPre pre,
                                              FinArgs fa) {
    static_assert(PRE || !RES, "the residual belongs to the deferred unit");
    __shared__ __attribute__((aligned(16))) float sW[256];   // [co][ci], zero padded
    __shared__ double sStat[NT / 64][32];
    const int tid = threadIdx.x;
    {
        const int co = tid >> 4, ci = tid & 15;
        sW[tid] = (co < Cout && ci < Cin) ? w[co * w_co + ci * w_ci] : 0.f;
    }
    __syncthreads();
    const int lane = tid & 63, n = lane & 15, q = lane >> 4;
    const long ntiles = (npos + 15) >> 4;
    const long wave = (long)blockIdx.x * (NT / 64) + (tid >> 6);
    long tile = wave * tiles_per_wave;
    const long tend = tile + tiles_per_wave < ntiles ? tile + tiles_per_wave : ntiles;
    const bool cin_ok = 4 * q < Cin, cout_ok = 4 * q < Cout;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (bias && cout_ok) bv = *reinterpret_cast<const f32x4*>(bias + 4 * q);
    if (shift && cout_ok) bv -= *reinterpret_cast<const f32x4*>(shift + 4 * q);
    PreConst pk{};
    float sl = 1.f;
    if constexpr (PRE) {
        pk = pre_const(pre, q, CinT);
        sl = pk.act ? pk.sl : 1.f;           // (no activation: z > 0 ? z : 1 * z is z)
    }
    const f32x4 A = *reinterpret_cast<const f32x4*>(sW + n * 16 + 4 * q);
    if (tile >= tend) goto finish;           // (a wave past the last tile still takes part in the reductions below)
    {
        // wave-uniform bases (scalar registers) + 32-bit lane offsets, both advanced per tile
        const long p0 = tile * 16;
        const float* inb = in;
        const float* resb = pre.res;
        float* aob = pre.a_out;
        float* outb = out;
        unsigned ioff = (unsigned)((p0 + n) * CinT + cin_off + 4 * q);      // elements; the tensors have < 2^31 of them
        unsigned ooff = (unsigned)((p0 + n) * Cout + 4 * q);
        const unsigned istep = 16u * (unsigned)CinT, ostep = 16u * (unsigned)Cout;
        long p = p0 + n;
        auto ld_in = [&](unsigned off) {
            if constexpr (FIN == 0) return *reinterpret_cast<const f32x4*>(inb + off);
            else {
                const u32x2 u = *reinterpret_cast<const u32x2*>(reinterpret_cast<const unsigned short*>(inb) + off);
                return uint2{u.x, u.y};
            }
        };
        // PW_U tiles per iteration, the NEXT PW_U already requested: 2 x PW_U tiles of input in flight per wave (one tile per
        // wave at a time left the kernel at ~3.4 TB/s: 16 waves per CU x 0.5-1 KB is a third of what the latency asks for)
        typename Raw4<FIN>::t cur[PW_U], nxt[PW_U];
        f32x4 rcur[PW_U], rnxt[PW_U];
        auto fetch = [&](long tl, long pp, unsigned off, typename Raw4<FIN>::t (&r)[PW_U], f32x4 (&rr)[PW_U]) {
#pragma unroll
            for (int u = 0; u < PW_U; ++u) {
                const bool ok = tl + u < tend && pp + 16 * u < npos;
                r[u] = ld_in((ok && cin_ok) ? off + (unsigned)u * istep : 0u);
                rr[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                if constexpr (RES) rr[u] = sld4(resb, ok ? (long)(off + (unsigned)u * istep) : 0L, FIN);
            }
        };
        fetch(tile, p, ioff, cur, rcur);
        for (; tile < tend; tile += PW_U) {
            if (tile + PW_U < tend) fetch(tile + PW_U, p + 16 * PW_U, ioff + PW_U * istep, nxt, rnxt);     // (wave-uniform)
            f32x4 xv[PW_U], acc[PW_U];
#pragma unroll
            for (int u = 0; u < PW_U; ++u) {
                const bool pv = tile + u < tend && p + 16 * u < npos;
                f32x4 d = dec4<FIN>(cur[u]);
                if constexpr (PRE) {
                    f32x4 a;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float z = pk.gm[e] * ((d[e] - pk.mean[e]) * pk.istd[e]) + pk.bt[e];
                        if constexpr (RES) z += rcur[u][e];
                        a[e] = z > 0.f ? z : sl * z;
                    }
                    d = round_bf4(a, FIN);
                    if (pv && aob) sst4<kNtSt>(aob, (long)(ioff + (unsigned)u * istep), FIN, d);
                }
                // (a lane past the last position computes on element 0's data and stores nothing: no select needed; the
                // channel quads past Cin -- point_conv1 reads 8 of 16 channels -- meet zero weight rows but must not bring
                // another tensor region's Inf / NaN to them)
                const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                if constexpr (PRE) xv[u] = d;
                else xv[u] = cin_ok ? d : zero;
                acc[u] = bv;
            }
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)           // the tiles' k-ordered chains interleaved
#pragma unroll
                for (int u = 0; u < PW_U; ++u) acc[u] = mfma4(A[s4], xv[u][s4], acc[u]);
#pragma unroll
            for (int u = 0; u < PW_U; ++u) {
                const bool pv = tile + u < tend && p + 16 * u < npos;
                if (pv && cout_ok) {
                    acc[u] = round_bf4(acc[u], OUTF);  // the statistics are those of the STORED tensor (the backward re-reads it)
                    sst4<kNtSt>(outb, (long)(ooff + (unsigned)u * ostep), OUTF, acc[u]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const double a = (double)acc[u][e]; s1[e] += a; s2[e] = fma(a, a, s2[e]); }
                }
            }
#pragma unroll
            for (int u = 0; u < PW_U; ++u) { cur[u] = nxt[u]; rcur[u] = rnxt[u]; }
            ioff += PW_U * istep;
            ooff += PW_U * ostep;
            p += 16 * PW_U;
        }
    }
finish:
    if (stat_partial) {          // as k_conv_mfma: lanes -> LDS -> one thread per (sum, channel), fixed order
#pragma unroll
        for (int e = 0; e < 4; ++e) { s1[e] = wave_sum_xor(s1[e], 1, 8); s2[e] = wave_sum_xor(s2[e], 1, 8); }
        if (n == 0)
#pragma unroll
            for (int e = 0; e < 4; ++e) { sStat[tid >> 6][4 * q + e] = s1[e]; sStat[tid >> 6][16 + 4 * q + e] = s2[e]; }
        __syncthreads();
        if (tid < 2 * Cout) {
            const int which = tid / Cout, ch = tid - which * Cout;
            double t = 0.0;
            for (int w2 = 0; w2 < NT / 64; ++w2) t += sStat[w2][which * 16 + ch];
            st_part(stat_partial + (long)blockIdx.x * 2 * Cout + tid, t, fa);
        }
        if (fa.kind) fin_reduce(stat_partial, 2 * Cout, blockIdx.x, gridDim.x, fa);
    }
}

// ------------------------------------------------ the two 16 -> 16 (1,5) stride-2 forward convs, dedicated form
// encoder.en_convs.1 (Conv2d, 65 -> 33 bins) and decoder.de_convs.3 (ConvTranspose2d, 33 -> 65 bins) ran through
// k_conv_mfma<1, 5>: 314 us each on 0.8 GB (2.6 TB/s), most of it the general kernel's per-tap bookkeeping (run-time
// stride / mode / parity logic, 64-bit row arithmetic, a (b, t, f) position carried per tile).  Same structure as
// k_pw_fwd: the bin counts are compile-time (row = p / FO is a multiply), offsets are 32-bit, the five A fragments
// stay in registers, all five tap loads of a tile are issued before the first MFMA.  Same taps in the same order
// (kf = 0 .. 4, a tap outside the row enters as zero), bias first, statistics in double: bit-identical outputs.
template <int FIN, int OUTF, bool TR>      // TR: the transposed conv (decoder)
__global__ __launch_bounds__(NT) void k_c15_fwd(long npos, int w_co, int w_ci, const float* __restrict__ in,
                                               const float* __restrict__ w, const float* __restrict__ bias,
                                               float* __restrict__ out, long tiles_per_wave, double* __restrict__ stat_partial,
                                               const float* __restrict__ shift, FinArgs fa) {
    constexpr unsigned FI = TR ? 33 : 65, FO = TR ? 65 : 33;
    __shared__ __attribute__((aligned(16))) float sW[5 * 256];   // [tap][co][ci]
    __shared__ double sStat[NT / 64][32];
    const int tid = threadIdx.x;
    for (int i = tid; i < 5 * 256; i += NT) {
        const int k = i >> 8, co = (i >> 4) & 15, ci = i & 15;
        sW[i] = w[co * w_co + ci * w_ci + k];
    }
    __syncthreads();
    const int lane = tid & 63, n = lane & 15, q = lane >> 4;
    const long ntiles = (npos + 15) >> 4;
    const long wave = (long)blockIdx.x * (NT / 64) + (tid >> 6);
    long tile = wave * tiles_per_wave;
    const long tend = tile + tiles_per_wave < ntiles ? tile + tiles_per_wave : ntiles;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (bias) bv = *reinterpret_cast<const f32x4*>(bias + 4 * q);
    if (shift) bv -= *reinterpret_cast<const f32x4*>(shift + 4 * q);
    f32x4 A[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) A[k] = *reinterpret_cast<const f32x4*>(sW + k * 256 + n * 16 + 4 * q);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if constexpr (TR) {
        // The transposed layer's outputs see only the taps of their own parity -- even bins kf = 0, 2, 4, odd bins kf = 1, 3:
        // with 16 consecutive bins per tile half of the 20 MFMAs and of the loads multiplied zeros (346 us).  Here a tile is
        // 16 outputs of ONE parity (all rows' even bins first, then all odd bins): 12 / 8 MFMAs, 3 / 2 loads, and the input
        // bins of a tile are consecutive.  Skipping a zero tap leaves the accumulator as it was: the same values.
        const unsigned rows = (unsigned)(npos / FO);
        const unsigned nE = rows * 33u, nO = rows * 32u, tE = (nE + 15u) >> 4, tO = (nO + 15u) >> 4;
        const unsigned ntl = tE + tO;
        const unsigned per = (ntl + (unsigned)gridDim.x * (NT / 64) - 1) / ((unsigned)gridDim.x * (NT / 64));
        unsigned tl = (unsigned)wave * per;
        const unsigned tl1 = tl + per < ntl ? tl + per : ntl;
        // (the next tile's loads are requested before this tile is computed: with one tile's three loads per wave in flight
        // the kernel waited a memory latency per tile -- 353 us for 0.8 GB; the two parities are two loops, so that the bins
        // per row and the tap count are compile-time inside each)
        auto run = [&](auto oddc, unsigned t0, unsigned t1, unsigned tbase, unsigned cnt) {
            constexpr bool ODD = decltype(oddc)::value;
            constexpr unsigned PER = ODD ? 32u : 33u;
            constexpr int NTAP = ODD ? 2 : 3;
            struct TIn { typename Raw4<FIN>::t raw[NTAP]; bool ok[NTAP]; bool pv; unsigned oidx; };
            auto fetch = [&](unsigned t_, TIn& ti) {
                const unsigned idx = (t_ - tbase) * 16u + n;
                ti.pv = idx < cnt;
                const unsigned row = idx / PER, j = idx - row * PER, f = 2u * j + (ODD ? 1u : 0u);
                const unsigned base = row * (FI * 16u) + 4u * q;
                ti.oidx = (row * FO + f) * 16u + 4u * q;
                // even: taps 0, 2, 4 read bins j + 1, j, j - 1; odd: taps 1, 3 read bins j + 1, j
#pragma unroll
                for (int u = 0; u < NTAP; ++u) {
                    const int fi = (int)j + 1 - u;
                    ti.ok[u] = ti.pv && fi >= 0 && fi < (int)FI;
                    ti.raw[u] = sld4_raw<FIN>(in, (long)(ti.ok[u] ? base + (unsigned)fi * 16u : 0u));
                }
            };
            TIn cur{}, nxt{};
            if (t0 < t1) fetch(t0, cur);
            for (unsigned t_ = t0; t_ < t1; ++t_) {
                nxt = cur;
                if (t_ + 1 < t1) fetch(t_ + 1, nxt);
                f32x4 acc = bv;
#pragma unroll
                for (int u = 0; u < NTAP; ++u) {
                    const f32x4 d = dec4<FIN>(cur.raw[u]);
                    const f32x4 xv = cur.ok[u] ? d : zero;
                    const f32x4 Ak = A[ODD ? 2 * u + 1 : 2 * u];
#pragma unroll
                    for (int s4 = 0; s4 < 4; ++s4) acc = mfma4(Ak[s4], xv[s4], acc);
                }
                if (cur.pv) {
                    acc = round_bf4(acc, OUTF);
                    sst4<kNtSt>(out, (long)cur.oidx, OUTF, acc);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const double a = (double)acc[e]; s1[e] += a; s2[e] = fma(a, a, s2[e]); }
                }
                cur = nxt;
            }
        };
        run(std::false_type{}, tl < tE ? tl : tE, tl1 < tE ? tl1 : tE, 0u, nE);
        run(std::true_type{}, tl > tE ? tl : tE, tl1 > tE ? tl1 : tE, tE, nO);
    }
    if constexpr (!TR) {
        unsigned p = (unsigned)(tile * 16) + n;          // (positions and element offsets fit in 31 bits: the launcher checks)
        const unsigned np32 = (unsigned)npos;
        struct EIn { typename Raw4<FIN>::t raw[5]; bool ok[5]; };
        auto fetch = [&](unsigned pp, EIn& ti) {
            const bool pv = pp < np32;
            const unsigned row = pp / FO, f = pp - row * FO, base = row * (FI * 16u) + 4u * q;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const int fi = 2 * (int)f - 2 + k;
                ti.ok[k] = pv && fi >= 0 && fi < (int)FI;
                ti.raw[k] = sld4_raw<FIN>(in, (long)(ti.ok[k] ? base + (unsigned)fi * 16u : 0u));
            }
        };
        EIn cur{}, nxt{};
        if (tile < tend) fetch(p, cur);
        for (; tile < tend; ++tile, p += 16) {
            nxt = cur;
            if (tile + 1 < tend) fetch(p + 16, nxt);       // (the next tile's five loads in flight while this one is computed)
            f32x4 acc = bv;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const f32x4 d = dec4<FIN>(cur.raw[k]);
                const f32x4 xv = cur.ok[k] ? d : zero;
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) acc = mfma4(A[k][s4], xv[s4], acc);
            }
            if (p < np32) {
                acc = round_bf4(acc, OUTF);      // the statistics are those of the STORED tensor (the backward re-reads it)
                sst4<kNtSt>(out, (long)(p * 16u + 4u * q), OUTF, acc);
#pragma unroll
                for (int e = 0; e < 4; ++e) { const double a = (double)acc[e]; s1[e] += a; s2[e] = fma(a, a, s2[e]); }
            }
            cur = nxt;
        }
    }
    if (stat_partial) {          // as k_conv_mfma
#pragma unroll
        for (int e = 0; e < 4; ++e) { s1[e] = wave_sum_xor(s1[e], 1, 8); s2[e] = wave_sum_xor(s2[e], 1, 8); }
        if (n == 0)
#pragma unroll
            for (int e = 0; e < 4; ++e) { sStat[tid >> 6][4 * q + e] = s1[e]; sStat[tid >> 6][16 + 4 * q + e] = s2[e]; }
        __syncthreads();
        if (tid < 32) {
            double t = 0.0;
            for (int w2 = 0; w2 < NT / 64; ++w2) t += sStat[w2][tid];
            st_part(stat_partial + (long)blockIdx.x * 32 + tid, t, fa);
        }
        if (fa.kind) fin_reduce(stat_partial, 32, blockIdx.x, gridDim.x, fa);
    }
}

// The window form on the VALU, for the FORWARD of encoder.en_convs.0: thread (position, channel quad), the window as
// four unaligned 16-byte loads (the four lanes of a position read the same addresses), then the multiply-adds of
// k_conv<3, 16> in ITS order (tap, input channel: one fp32 fmaf chain per output channel; a tap outside the row enters
// as x = 0).  The conv outputs are therefore bit-identical to the reference-ordered kernel -- which matters here: with
// the random-weight fixture a pre-activation further down sits within an fp32 ulp of a PReLU kink, the MFMA window
// form above (same values, other summation order) lands on the reference's side of it, and the gradients then differ
// from the float64 truth exactly as the reference's do (1.6e-3 of a tensor's scale) instead of by 1.1e-4
// (tests/test_gpu_train.py::test_gradients_against_fp64_truth).  626 -> ~200 us at B = 512.
template <int FIN>
// (launch bound: 4 workgroups per CU, so that the 1024-workgroup grid is resident in one round)
__global__ __launch_bounds__(NT, 4) void k_conv_win_fma(ConvGeom g, const float* __restrict__ in, const float* __restrict__ w,
                                                    const float* __restrict__ bias, float* __restrict__ out,
                                                    double* __restrict__ stat_partial, StrideIter it,
                                                    const float* __restrict__ shift, FinArgs fa) {
    __shared__ __attribute__((aligned(16))) float sW[256];   // [j][co], j = kf * Cin + ci
    __shared__ double sStat[NT / 64][32];
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};    // in double: see k_conv_mfma
    const int tid = threadIdx.x;
    {
        const int j = tid >> 4, co = tid & 15, kf = j / g.Cin, ci = j - kf * g.Cin;
        sW[tid] = (kf < g.nkf && co < g.Cout) ? w[co * g.w_co + ci * g.w_ci + kf * g.w_kf] : 0.f;
    }
    __syncthreads();
    const long units = (long)g.B * g.Tout * g.Fout * 4;
    const int q = tid & 3, J = g.Cin * g.nkf;
    const long rowlen = (long)g.Fin * g.Cin, total = (long)g.B * g.Tin * rowlen;
    RowPos P;
    P.init(((long)blockIdx.x * NT + tid) >> 2, g.Fout, g.Tout);
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (bias) bv = *reinterpret_cast<const f32x4*>(bias + 4 * q);
    if (shift) bv -= *reinterpret_cast<const f32x4*>(shift + 4 * q);
    for (long i = (long)blockIdx.x * NT + tid; i < units; i += (long)gridDim.x * NT) {
        const long p = i >> 2;
        const int e0 = (P.fo * g.sf - g.pf) * g.Cin;
        const long base = (long)P.bt * rowlen + e0;
        typename Raw4<FIN>::t raw[4];
        bool inside[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            inside[v] = base + 4 * v >= 0 && base + 4 * v + 4 <= total;
            raw[v] = sldw_raw<FIN>(in, inside[v] ? base + 4 * v : 0L);
        }
        float x[16];
        bool slow = false;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const f32x4 d = dec4<FIN>(raw[v]);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int j = 4 * v + s;
                const bool ok = j < J && e0 + j >= 0 && e0 + j < rowlen;
                x[j] = (ok && inside[v]) ? d[s] : 0.f;
                slow = slow || (ok && !inside[v]);
            }
        }
        if (slow) {      // a window that leaves the tensor: the first / last position of the whole tensor only -- ONE branch
                         // (an `if` per element put each of the sixteen in a basic block of its own: 82 exec-mask regions)
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const bool ok = j < J && e0 + j >= 0 && e0 + j < rowlen;
                if (ok && !inside[j >> 2]) x[j] = sld1(in, base + j, FIN);
            }
        }
        f32x4 acc = bv;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const f32x4 wt = *reinterpret_cast<const f32x4*>(sW + j * 16 + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(wt[e], x[j], acc[e]);
        }
        P.advance(it, g.Fout, g.Tout);
        if (g.out_bf) {
            acc = round_bf4(acc, g.out_bf);
            sst4<kNtSt>(out, p * 16 + 4 * q, g.out_bf, acc);
        } else {
            sst4<kNtSt>(out, p * 16 + 4 * q, 0, acc);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) { const double a = (double)acc[e]; s1[e] += a; s2[e] = fma(a, a, s2[e]); }
    }
    if (stat_partial) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { s1[e] = wave_sum_xor(s1[e], 4, 32); s2[e] = wave_sum_xor(s2[e], 4, 32); }
        if ((tid & 63) < 4)
#pragma unroll
            for (int e = 0; e < 4; ++e) { sStat[tid >> 6][4 * q + e] = s1[e]; sStat[tid >> 6][16 + 4 * q + e] = s2[e]; }
        __syncthreads();
        if (tid < 32) {
            double t = 0.0;
            for (int w2 = 0; w2 < NT / 64; ++w2) t += sStat[w2][tid];
            st_part(stat_partial + (long)blockIdx.x * 32 + tid, t, fa);
        }
        if (fa.kind) fin_reduce(stat_partial, 32, blockIdx.x, gridDim.x, fa);
    }
}

constexpr int WG_WAVES = 4;   // waves per workgroup of the MFMA weight-gradient kernel
template <int NKT, int NKF, int FMT>   // FMT: storage format of `in`, compile time (see sld1)
__global__ __launch_bounds__(WG_WAVES * 64) void k_conv_wgrad_mfma(ConvGeom g, const float* __restrict__ in,
                                                                  const float* __restrict__ dout,
                                                                  float* __restrict__ partial,
                                                                  long groups_per_wave) {
    constexpr int NTAP = NKT * NKF;
    __shared__ float sAcc[WG_WAVES][NTAP * 256 + 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, k = lane >> 4;
    const long npos = (long)g.B * g.Tout * g.Fout, ngroups = (npos + 3) >> 2;
    const long wave = (long)blockIdx.x * WG_WAVES + wv;
    long grp = wave * groups_per_wave;
    const long gend = grp + groups_per_wave < ngroups ? grp + groups_per_wave : ngroups;
    f32x4 acc[NTAP];
#pragma unroll
    for (int i = 0; i < NTAP; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    if (grp < gend) {
        Pos P;
        {
            const long p0 = grp * 4 + k;
            P.init(p0 < npos ? p0 : npos - 1, g.Fout, g.Tout);
        }
        const bool co_ok = c < g.Cout, ci_ok = c < g.Cin;
        constexpr int U = 4;      // groups per iteration: all their loads are issued before the first MFMA
        for (; grp < gend; grp += U) {
            float a[U];
            unsigned bb[U][NTAP];        // raw words: decoded after all loads are in flight
            unsigned odd[U];             // bit tap: the element is the high half of its word (16-bit formats)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long p = (grp + u) * 4 + k;
                const bool pv = p < npos && grp + u < gend;
                a[u] = (pv && co_ok) ? dout[p * g.CoutT + g.cout_off + c] : 0.f;
                odd[u] = 0;
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt) {
                    const int ti = P.t + g.t_off[kt];
                    const bool okt = pv && ci_ok && ti >= 0 && ti < g.Tin;
                    const long rowbase = ((long)P.b * g.Tin + ti) * g.Fin;
#pragma unroll
                    for (int kf = 0; kf < NKF; ++kf) {
                        int fi;
                        const bool ok = tap_fi(g, P.f, kf, fi) && okt;
                        const long ix = (rowbase + fi) * g.CinT + g.cin_off + c;
                        odd[u] |= (unsigned)(ix & 1) << (kt * NKF + kf);
                        bb[u][kt * NKF + kf] = ok ? sld1_raw<FMT>(in, ix) : 0u;
                    }
                }
                P.advance(4, g.Fout, g.Tout);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                bsum += a[u];
#pragma unroll
                for (int tap = 0; tap < NTAP; ++tap) acc[tap] = mfma4(a[u], sld1_dec<FMT>(bb[u][tap], (odd[u] >> tap) & 1u), acc[tap]);
            }
        }
    }
    // D fragment: lane (j = c, q = k) holds dW[co = 4q + r][ci = j] of each tap
#pragma unroll
    for (int tap = 0; tap < NTAP; ++tap)
#pragma unroll
        for (int r = 0; r < 4; ++r) sAcc[wv][tap * 256 + (4 * k + r) * 16 + c] = acc[tap][r];
    sAcc[wv][NTAP * 256 + lane] = bsum;
    __syncthreads();
    float* pp = partial + (long)blockIdx.x * (NTAP * 256 + 16);
    for (int i = tid; i < NTAP * 256; i += WG_WAVES * 64) {
        float s = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < WG_WAVES; ++w2) s += sAcc[w2][i];
        pp[i] = s;
    }
    if (tid < 16) {
        float s = 0.f;
        for (int w2 = 0; w2 < WG_WAVES; ++w2)
            for (int kk = 0; kk < 4; ++kk) s += sAcc[w2][NTAP * 256 + kk * 16 + tid];
        pp[NTAP * 256 + tid] = s;
    }
}

// The same weight gradient with 16-byte operand loads (round 3).  k_conv_wgrad_mfma above feeds the MFMA from 4-byte
// loads -- lane (c, k) fetches channel c of position 4 group + k, a wave-instruction moves 256 bytes -- and ran at
// 0.8-1.0 TB/s of operand bytes: request-bound.  Here a wave takes 16 positions per trip: lane (n, q) loads channels
// 4q..4q+3 of position n of dout and of every tap-shifted input (ONE 16-byte load each, 1 KB per wave-instruction,
// all issued before anything is used), parks the (1 + taps) tiles in its own 1 KB LDS slots and reads the MFMA
// operands back as scalars -- lane (c, k) takes [4u + k][c]: 64 different banks.  Same operands into the same MFMA
// sequence as above: bit-identical partial sums.
template <int NKT, int NKF, int FMT>
__global__ __launch_bounds__(WG_WAVES * 64) void k_conv_wgrad_lds(ConvGeom g, const float* __restrict__ in,
                                                                 const float* __restrict__ dout,
                                                                 float* __restrict__ partial, long groups_per_wave) {
    constexpr int NTAP = NKT * NKF;
    constexpr int SLOT = (1 + NTAP) * 256 > NTAP * 256 + 64 ? (1 + NTAP) * 256 : NTAP * 256 + 64;
    __shared__ __attribute__((aligned(16))) float sT[WG_WAVES][SLOT];   // per wave: operand tiles, later its accumulators
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, k = lane >> 4;   // = (n, q) for the loads
    float* my = sT[wv];
    const long npos = (long)g.B * g.Tout * g.Fout, ngroups = (npos + 3) >> 2;
    const long wave = (long)blockIdx.x * WG_WAVES + wv;
    long grp = wave * groups_per_wave;
    const long gend = grp + groups_per_wave < ngroups ? grp + groups_per_wave : ngroups;
    f32x4 acc[NTAP];
#pragma unroll
    for (int i = 0; i < NTAP; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    if (grp < gend) {
        Pos P;
        {
            const long p0 = grp * 4 + c;
            P.init(p0 < npos ? p0 : npos - 1, g.Fout, g.Tout);
        }
        const bool co_ok = 4 * k < g.Cout, ci_ok = 4 * k < g.Cin;
        for (; grp < gend; grp += 4) {
            const long p = grp * 4 + c;                          // this lane's position of the 16
            const bool pv = p < npos && grp + (c >> 2) < gend;
            f32x4 a4 = {0.f, 0.f, 0.f, 0.f};
            typename Raw4<FMT>::t raw[NTAP];
            if (pv && co_ok) a4 = *reinterpret_cast<const f32x4*>(dout + p * g.CoutT + g.cout_off + 4 * k);
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) {
                const int ti = P.t + g.t_off[kt];
                const bool okt = pv && ci_ok && ti >= 0 && ti < g.Tin;
                const long rowbase = ((long)P.b * g.Tin + ti) * g.Fin;
#pragma unroll
                for (int kf = 0; kf < NKF; ++kf) {
                    int fi;
                    const bool ok = tap_fi_t<NKF != 5>(g, P.f, kf, fi) && okt;
                    typename Raw4<FMT>::t z{};
                    raw[kt * NKF + kf] = ok ? sld4_raw<FMT>(in, (rowbase + fi) * g.CinT + g.cin_off + 4 * k) : z;
                }
            }
            P.advance(16, g.Fout, g.Tout);
            *reinterpret_cast<f32x4*>(my + c * 16 + 4 * k) = a4;
#pragma unroll
            for (int tap = 0; tap < NTAP; ++tap)
                *reinterpret_cast<f32x4*>(my + (1 + tap) * 256 + c * 16 + 4 * k) = dec4<FMT>(raw[tap]);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float a = my[(4 * u + k) * 16 + c];
                bsum += a;
#pragma unroll
                for (int tap = 0; tap < NTAP; ++tap) acc[tap] = mfma4(a, my[(1 + tap) * 256 + (4 * u + k) * 16 + c], acc[tap]);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    // D fragment: lane (j = c, q = k) holds dW[co = 4q + r][ci = j] of each tap (the wave's own slot: its tiles are dead)
#pragma unroll
    for (int tap = 0; tap < NTAP; ++tap)
#pragma unroll
        for (int r = 0; r < 4; ++r) my[tap * 256 + (4 * k + r) * 16 + c] = acc[tap][r];
    my[NTAP * 256 + lane] = bsum;
    __syncthreads();
    float* pp = partial + (long)blockIdx.x * (NTAP * 256 + 16);
    for (int i = tid; i < NTAP * 256; i += WG_WAVES * 64) {
        float s = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < WG_WAVES; ++w2) s += sT[w2][i];
        pp[i] = s;
    }
    if (tid < 16) {
        float s = 0.f;
        for (int w2 = 0; w2 < WG_WAVES; ++w2)
            for (int kk = 0; kk < 4; ++kk) s += sT[w2][NTAP * 256 + kk * 16 + tid];
        pp[NTAP * 256 + tid] = s;
    }
}

// Weight gradient of the two narrow layers in window form (see win_pos): dW[wide channel][j] = sum over the 16-channel
// positions of wide[p][c] * window(p)[j], one MFMA per four positions.  WIDE_IN: the 16-channel operand is `in`
// (transposed conv, de_convs.4: the window is over dout), otherwise dout (en_convs.0: the window is over `in`).
// Both operands arrive as 16-byte loads in the (position, quad) layout and go through the wave's LDS tiles into the
// (channel, position) layout of the MFMA operands, as in k_conv_wgrad_lds.
// partial per workgroup: [16][16] dW, 16 sums of the wide operand per channel, 16 sums of the window per element.
template <int FMT, bool WIDE_IN>
__global__ __launch_bounds__(WG_WAVES * 64) void k_wgrad_win(ConvGeom g, const float* __restrict__ in,
                                                            const float* __restrict__ dout,
                                                            float* __restrict__ partial, long groups_per_wave) {
    constexpr int FW = WIDE_IN ? FMT : 0, FN = WIDE_IN ? 0 : FMT;
    __shared__ __attribute__((aligned(16))) float sT[WG_WAVES][512];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, k = lane >> 4;   // = (n, q) for the loads
    float* my = sT[wv];
    const float* wide = WIDE_IN ? in : dout;
    const float* nar = WIDE_IN ? dout : in;
    const int Cn = WIDE_IN ? g.Cout : g.Cin, Fw = WIDE_IN ? g.Fin : g.Fout, Fn = WIDE_IN ? g.Fout : g.Fin;
    const int J = Cn * g.nkf;
    const long rowlen = (long)Fn * Cn, total = (long)g.B * g.Tin * rowlen;
    const long npos = (long)g.B * g.Tin * Fw, ngroups = (npos + 3) >> 2;
    const long wave = (long)blockIdx.x * WG_WAVES + wv;
    long grp = wave * groups_per_wave;
    const long gend = grp + groups_per_wave < ngroups ? grp + groups_per_wave : ngroups;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float asum = 0.f, bsum = 0.f;
    if (grp < gend) {
        Pos P;
        {
            const long p0 = grp * 4 + c;
            P.init(p0 < npos ? p0 : npos - 1, Fw, g.Tin);
        }
        for (; grp < gend; grp += 4) {
            const long p = grp * 4 + c;                          // this lane's position of the 16
            const bool pv = p < npos && grp + (c >> 2) < gend;
            const typename Raw4<FW>::t wraw = sld4_raw<FW>(wide, pv ? p * 16 + 4 * k : 0L);
            const WinPos wp = win_pos(P, pv, k, Cn, J, g.sf, g.pf, g.Tin, rowlen, total);
            const typename Raw4<FN>::t nraw = sldw_raw<FN>(nar, (wp.any && !wp.edge) ? wp.idx : 0L);
            P.advance(16, Fw, g.Tin);
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            const f32x4 wd = dec4<FW>(wraw);
            *reinterpret_cast<f32x4*>(my + c * 16 + 4 * k) = pv ? wd : zero;
            *reinterpret_cast<f32x4*>(my + 256 + c * 16 + 4 * k) = win_value<FN>(nar, wp, nraw);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float a = my[(4 * u + k) * 16 + c], b = my[256 + (4 * u + k) * 16 + c];
                asum += a;
                bsum += b;
                acc = mfma4(a, b, acc);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    // D fragment: lane (j = c, q = k) holds dW[wide channel 4q + r][j]
#pragma unroll
    for (int r = 0; r < 4; ++r) my[(4 * k + r) * 16 + c] = acc[r];
    my[256 + lane] = asum;
    my[320 + lane] = bsum;
    __syncthreads();
    float* pp = partial + (long)blockIdx.x * 288;
    {
        float s = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < WG_WAVES; ++w2) s += sT[w2][tid];
        pp[tid] = s;
    }
    if (tid < 32) {
        const int base = tid < 16 ? 256 : 320, ch = tid & 15;
        float s = 0.f;
        for (int w2 = 0; w2 < WG_WAVES; ++w2)
            for (int kk = 0; kk < 4; ++kk) s += sT[w2][base + kk * 16 + ch];
        pp[256 + tid] = s;
    }
}
// partial [nparts][288] -> dw (reference layout), dbias.  The bias gradient is the sum of dout over ITS positions: the
// wide operand's channel sums when dout is the wide one; otherwise the window elements of taps 2 and 3 (narrow bins
// 2f and 2f+1: every bin exactly once over the positions f of a row)
__global__ __launch_bounds__(1024) void k_wgrad_win_finish(ConvGeom g, const float* __restrict__ partial, int nparts,
                                                          float* __restrict__ dw, float* __restrict__ dbias,
                                                          int wide_in) {
    __shared__ double sh[16][64];
    __shared__ double tot[64];
    const int K = 288;
    const int j = threadIdx.x & 63, slice = threadIdx.x >> 6, k = blockIdx.x * 64 + j;
    double s = k < K ? sum_strided(partial + k, slice, nparts, 16, K) : 0.0;
    sh[slice][j] = s;
    __syncthreads();
    if (slice == 0) {
        for (int q = 1; q < 16; ++q) s += sh[q][j];
        tot[j] = s;
    }
    __syncthreads();
    if (slice != 0 || k >= K) return;
    const int Cn = wide_in ? g.Cout : g.Cin;
    if (k < 256) {
        const int wc = k >> 4, jj = k & 15, kf = jj / Cn, cn = jj - kf * Cn;
        const int co = wide_in ? cn : wc, ci = wide_in ? wc : cn;
        if (kf < g.nkf && co < g.Cout && ci < g.Cin) dw[co * g.w_co + ci * g.w_ci + kf * g.w_kf] = (float)s;
    } else if (dbias) {
        const int r = k - 256;            // 0..15: wide channel sums, 16..31: window element sums (same block: tot[])
        if (!wide_in && r < g.Cout) dbias[r] = (float)s;
        if (wide_in && r >= 16 && r - 16 < g.Cout) dbias[r - 16] = (float)(tot[j + 2 * Cn] + tot[j + 3 * Cn]);
    }
}

// partial [nparts][ntap*256 + 16] -> dw (reference layout), dbias.  1024 threads = 64 outputs x 16 slices
// of the partials; the slices are combined in a fixed order.
__global__ __launch_bounds__(1024) void k_wgrad_mfma_finish(ConvGeom g, const float* __restrict__ partial, int nparts,
                                                           float* __restrict__ dw, float* __restrict__ dbias) {
    __shared__ double sh[16][64];
    const int ntap = g.nkt * g.nkf, K = ntap * 256 + 16;
    const int j = threadIdx.x & 63, slice = threadIdx.x >> 6, k = blockIdx.x * 64 + j;
    double s = k < K ? sum_strided(partial + k, slice, nparts, 16, K) : 0.0;
    sh[slice][j] = s;
    __syncthreads();
    if (slice != 0 || k >= K) return;
    for (int q = 1; q < 16; ++q) s += sh[q][j];
    if (k >= ntap * 256) {
        const int co = k - ntap * 256;
        if (dbias && co < g.Cout) dbias[co] = (float)s;
    } else {
        const int tap = k >> 8, co = (k >> 4) & 15, ci = k & 15, kt = tap / g.nkf, kf = tap - kt * g.nkf;
        if (co < g.Cout && ci < g.Cin) dw[co * g.w_co + ci * g.w_ci + kt * g.w_kt + kf * g.w_kf] = (float)s;
    }
}

// -------------------------------------------------------------------------- depthwise conv
// SFE_Lite (:77-90), encoder depth_conv groups=16 (:206-216), TCN conv2 (:273-281), + data gradients
template <int C>
__global__ __launch_bounds__(NT) void k_dw(DwGeom g, const float* __restrict__ in, const float* __restrict__ w,
                                          const float* __restrict__ bias, float* __restrict__ out) {   // (no BatchNorm follows the 3-channel SFE conv: no shift)
    __shared__ float sW[9 * C];   // [tap][c]
    const int tid = threadIdx.x, ntap = g.nkt * g.nkf;
    for (int i = tid; i < ntap * C; i += NT) {
        const int tap = i / C, c = i - tap * C, kt = tap / g.nkf, kf = tap - kt * g.nkf;
        sW[i] = w[c * g.w_c + kt * g.w_kt + kf * g.w_kf];
    }
    __syncthreads();
    const long npos = (long)g.B * g.Tout * g.F;
    for (long p = (long)blockIdx.x * NT + tid; p < npos; p += (long)gridDim.x * NT) {
        const int fo = (int)(p % g.F);
        const long bt = p / g.F;
        const int to = (int)(bt % g.Tout), b = (int)(bt / g.Tout);
        float acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = bias ? bias[c] : 0.f;
        for (int kt = 0; kt < g.nkt; ++kt) {
            const int ti = to + g.t_off[kt];
            if (ti < 0 || ti >= g.Tin) continue;
            for (int kf = 0; kf < g.nkf; ++kf) {
                const int fi = fo + g.f_off[kf];
                if (fi < 0 || fi >= g.F) continue;
                float xv[C];
                load_vec_s<C>(in, (((long)b * g.Tin + ti) * g.F + fi) * C, g.in_bf, xv);
                const float* wt = sW + (kt * g.nkf + kf) * C;
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] = fmaf(wt[c], xv[c], acc[c]);
            }
        }
        if (g.out2) {
#pragma unroll
            for (int c = 0; c < C; ++c) { out[p * C + c] = acc[c]; sst1(g.out2, p * C + c, g.out2_bf, acc[c]); }
        } else if (g.out_bf) {
#pragma unroll
            for (int c = 0; c < C; ++c) sst1(out, p * C + c, g.out_bf, acc[c]);
        } else {
            float* o = out + p * C;
#pragma unroll
            for (int c = 0; c < C; ++c) o[c] = g.accumulate ? o[c] + acc[c] : acc[c];
        }
    }
}

// C = 16: one thread per (position, 4 channels): every tap is one coalesced 16-byte load
// NKT x NKF: the tap grid as compile-time constants (3x3 encoder depth convs, 3x1 dilated TCN convs and their adjoints);
// 0 x 0: run-time tap counts (any other shape)
// FIN: storage format of `in` as a compile-time constant (-1: run-time g.in_bf): with the run-time flag the 16-bit
// branch of every tap load decodes inside its own basic block, i.e. waits for that load before the next one is issued
// (bf16 storage: k_dw16<3,3> 245 us against 165 with fp32 storage, twice the bytes)
// PRE: `in` is the previous unit's conv output (see BnPre); the last temporal / middle frequency tap is the thread's
// own position (t_off[NKT-1] == 0, f_off[NKF/2] == 0: checked by the launcher) and stores the activation
template <int NV, int V, class TV>
__device__ __forceinline__ void block_reduce_store(const TV (&v)[NV][V], int C, double* sh, double* dst, bool pub = false);
// NEXT: see k_conv_mfma
template <int NKT, int NKF, int FIN = -1, bool PRE = false, int NEXT = 0>
__global__ __launch_bounds__(NT) void k_dw16(DwGeom g, const float* __restrict__ in, const float* __restrict__ w,
                                            const float* __restrict__ bias, float* __restrict__ out,
                                            double* __restrict__ stat_partial, StrideIter it,
                                            const float* __restrict__ shift, BnPre pre, NextRedArgs nx, FinArgs fa) {
    const unsigned vb = xcd_block();
    static_assert(!NEXT || (!PRE && NKT > 0), "riding reduction: plain adjoint launches");
    NextConst nk{};
    float vr[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) vr[0][e] = vr[1][e] = vr[2][e] = 0.f;
    if constexpr (NEXT) nk = next_const(nx, 4 * (threadIdx.x & 3));
    static_assert(!PRE || (FIN >= 0 && NKT > 0), "normalise-on-load needs the compile-time forms");
    __shared__ __attribute__((aligned(16))) float sW[9 * 16];   // [tap][c]
    __shared__ double sStat[NT / 64][32];   // per wave: sum[16], sum of squares[16]
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};    // in double: see k_conv_mfma
    const int tid = threadIdx.x, ntap = g.nkt * g.nkf;
    for (int i = tid; i < ntap * 16; i += NT) {
        const int tap = i >> 4, c = i & 15, kt = tap / g.nkf, kf = tap - kt * g.nkf;
        sW[i] = w[c * g.w_c + kt * g.w_kt + kf * g.w_kf];
    }
    __syncthreads();
    // Tin == Tout for every depthwise conv of the model, so the tap row is (flat row + t_off): no (b, t) split
    const long units = (long)g.B * g.Tout * g.F * 4;
    const int q = tid & 3;
    PreConst pk{};
    if constexpr (PRE) pk = pre_const(pre, q, 16);
    RowPos P;
    P.init(((long)vb * NT + tid) >> 2, g.F, g.Tout);
    for (long i = (long)vb * NT + tid; i < units; i += (long)gridDim.x * NT) {
        const long p = i >> 2;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (bias) acc = *reinterpret_cast<const f32x4*>(bias + 4 * q);
        if (shift) acc -= *reinterpret_cast<const f32x4*>(shift + 4 * q);
        f32x4 ynx = {0.f, 0.f, 0.f, 0.f};
        if constexpr (NEXT) ynx = dec4<NEXT ? NEXT - 1 : 0>(sld4_raw<NEXT ? NEXT - 1 : 0, true>(nx.y, p * 16 + 4 * q));
        if constexpr (NKT > 0) {
            // every tap's load is issued before the first multiply-add (a tap outside the tensor loads the centre
            // record instead and is skipped by a select: one basic block, NKT * NKF loads in flight per thread instead
            // of one behind each branch); same taps, same order of additions as the loop form
            constexpr int FR = FIN < 0 ? 0 : FIN;
            f32x4 xv[NKT * NKF];
            typename Raw4<FR>::t xr[NKT * NKF];
            bool ok[NKT * NKF];
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int kf = 0; kf < NKF; ++kf) {
                    const int ti = P.to + g.t_off[kt], fi = P.fo + g.f_off[kf];
                    const bool v = ti >= 0 && ti < g.Tin && fi >= 0 && fi < g.F;
                    ok[kt * NKF + kf] = v;
                    const long rec = v ? (long)(P.bt + g.t_off[kt]) * g.F + fi : p;
                    if constexpr (FIN < 0) xv[kt * NKF + kf] = sld4(in, rec * 16 + 4 * q, g.in_bf);
                    else xr[kt * NKF + kf] = sld4_raw<FR>(in, rec * 16 + 4 * q);
                }
#pragma unroll
            for (int tp = 0; tp < NKT * NKF; ++tp) {
                if constexpr (FIN >= 0) xv[tp] = dec4<FR>(xr[tp]);
                if constexpr (PRE) {
                    const f32x4 yraw = xv[tp];
                    xv[tp] = pre_apply(pk, xv[tp], pre.exact ? 0 : pre.bf);
                    if (tp == (NKT - 1) * NKF + NKF / 2) {
                        pre_store(pre, p * 16 + 4 * q, xv[tp]);
                        pre_store_y(pre, pk, p * 16 + 4 * q, yraw, false, f32x4{0.f, 0.f, 0.f, 0.f});
                    }
                }
                const f32x4 wt = *reinterpret_cast<const f32x4*>(sW + tp * 16 + 4 * q);
                const f32x4 nx = acc + wt * xv[tp];
                acc = ok[tp] ? nx : acc;
            }
        } else {
            for (int kt = 0; kt < g.nkt; ++kt) {
                const int ti = P.to + g.t_off[kt];
                if (ti < 0 || ti >= g.Tin) continue;
                for (int kf = 0; kf < g.nkf; ++kf) {
                    const int fi = P.fo + g.f_off[kf];
                    if (fi < 0 || fi >= g.F) continue;
                    const f32x4 x = sld4(in, ((long)(P.bt + g.t_off[kt]) * g.F + fi) * 16 + 4 * q, g.in_bf);
                    const f32x4 wt = *reinterpret_cast<const f32x4*>(sW + (kt * g.nkf + kf) * 16 + 4 * q);
                    acc += wt * x;
                }
            }
        }
        P.advance(it, g.F, g.Tout);
        if (g.out_bf) {
            if (g.accumulate) acc = sld4(out, p * 16 + 4 * q, g.out_bf) + acc;
            acc = round_bf4(acc, g.out_bf);
            sst4<kNtSt>(out, p * 16 + 4 * q, g.out_bf, acc);
        } else {
            f32x4* o = reinterpret_cast<f32x4*>(out + p * 16 + 4 * q);
            if (g.accumulate) { acc = *o + acc; *o = acc; }
            else sst4<kNtSt>(out, p * 16 + 4 * q, 0, acc);
        }
        if constexpr (NEXT) next_accum(nk, ynx, acc, vr);
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e) { const double a = (double)acc[e]; s1[e] += a; s2[e] = fma(a, a, s2[e]); }
        }
    }
    if constexpr (NEXT) {
        __shared__ double shn[NT];
        block_reduce_store<3, 4>(vr, 16, shn, stat_partial + (long)vb * 48, fa.kind != 0);
        if (fa.kind) fin_reduce(stat_partial, 48, (int)vb, gridDim.x, fa);
        return;
    }
    if (stat_partial) {   // per-workgroup BatchNorm partial sums; a thread's channel quad is tid & 3
#pragma unroll
        for (int e = 0; e < 4; ++e) { s1[e] = wave_sum_xor(s1[e], 4, 32); s2[e] = wave_sum_xor(s2[e], 4, 32); }
        if ((tid & 63) < 4)
#pragma unroll
            for (int e = 0; e < 4; ++e) { sStat[tid >> 6][4 * q + e] = s1[e]; sStat[tid >> 6][16 + 4 * q + e] = s2[e]; }
        __syncthreads();
        if (tid < 32) {
            double t = 0.0;
            for (int w = 0; w < NT / 64; ++w) t += sStat[w][tid];
            st_part(stat_partial + (long)vb * 32 + tid, t, fa);
        }
        if (fa.kind) fin_reduce(stat_partial, 32, (int)vb, gridDim.x, fa);
    }
}

// ------------------------------------------- the TCN's dilated depthwise (3,1) conv behind a deferred unit, column form
// k_dw16<3, 1, FIN, PRE> gives a thread one (position, channel quad): it loads the taps t - 2d, t - d, t and applies the
// previous unit's BatchNorm + PReLU + rounding to ALL THREE -- every element of the input is normalised three times, by
// three different threads -- with three 8-byte loads in flight per thread: 141 us on 272 MB of bf16 tensors (1.9 TB/s).
// Here a thread owns a (b, f, channel quad) COLUMN and walks the frames of ONE residue class modulo the dilation,
// t = r + j d: the two older taps of output j are the thread's own values j - 2 and j - 1, so every input element is
// loaded and normalised once (a chunk of DC_J outputs re-reads the two values in front of it), and all DC_J + 2 loads of a
// chunk are requested before the first is used.  Same expressions in the same order per output as k_dw16 (bias - shift
// first, taps oldest first, a tap in front of the utterance skipped, statistics in double from the stored value): the
// conv outputs are bit-identical; the BatchNorm partial sums are taken in another order (double sums, the statistics round
// to the same floats: test_pass_fusions_... compares the masks bit for bit).
template <int FIN> struct DcChunk { static constexpr int J = FIN ? 16 : 8; };   // (fp32 raws are twice the registers: 4 waves per SIMD either way)
template <int FIN, int OUTF>
__global__ __launch_bounds__(NT) void k_dw31_col(int B, int T, int F, int d, int w_c, int w_kt, const float* __restrict__ in,
                                                const float* __restrict__ w, const float* __restrict__ bias,
                                                float* __restrict__ out, double* __restrict__ stat_partial,
                                                const float* __restrict__ shift, BnPre pre, FinArgs fa) {
    constexpr int DC_J = DcChunk<FIN>::J;
    __shared__ double sStat[NT / 64][32];
    const int tid = threadIdx.x, q = tid & 3;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    const PreConst pk = pre_const(pre, q, 16);
    f32x4 wt[3];
#pragma unroll
    for (int kt = 0; kt < 3; ++kt)
#pragma unroll
        for (int e = 0; e < 4; ++e) wt[kt][e] = w[(4 * q + e) * w_c + kt * w_kt];
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (bias) bv = *reinterpret_cast<const f32x4*>(bias + 4 * q);
    if (shift) bv -= *reinterpret_cast<const f32x4*>(shift + 4 * q);
    const int F4 = F * 4, S = ((T + d - 1) / d + DC_J - 1) / DC_J;     // chunks of a residue class
    const long items = (long)B * d * S * F4;
    const unsigned rowstep = (unsigned)d * (unsigned)F * 16u;          // elements between consecutive frames of a chain
    for (long item = (long)blockIdx.x * NT + tid; item < items; item += (long)gridDim.x * NT) {
        const int fq = (int)(item % F4);
        long rest = item / F4;
        const int sc = (int)(rest % S);
        rest /= S;
        const int r = (int)(rest % d), b = (int)(rest / d);
        const int j0 = sc * DC_J, t0 = r + j0 * d;
        if (t0 >= T) continue;
        // element offset of (b, t0, f, 4q); < 2^31 (the launcher checks)
        const unsigned off0 = (unsigned)(((long)b * T + t0) * F * 16 + fq * 4);
        typename Raw4<FIN>::t raw[DC_J + 2];
#pragma unroll
        for (int k = 0; k < DC_J + 2; ++k) {
            const int t = t0 + (k - 2) * d;
            const bool ok = t >= 0 && t < T;
            raw[k] = sld4_raw<FIN>(in, (long)(ok ? off0 + (unsigned)(k - 2) * rowstep : off0));
        }
        f32x4 x2 = pre_apply(pk, dec4<FIN>(raw[0]), FIN), x1 = pre_apply(pk, dec4<FIN>(raw[1]), FIN);
#pragma unroll
        for (int k = 0; k < DC_J; ++k) {
            const int t = t0 + k * d;
            const f32x4 x0 = pre_apply(pk, dec4<FIN>(raw[k + 2]), FIN);
            if (t < T) {
                const unsigned off = off0 + (unsigned)k * rowstep;
                if (pre.a_out) sst4<kNtSt>(pre.a_out, (long)off, FIN, x0);
                f32x4 acc = bv;
                const f32x4 n2 = acc + wt[0] * x2;
                acc = t - 2 * d >= 0 ? n2 : acc;
                const f32x4 n1 = acc + wt[1] * x1;
                acc = t - d >= 0 ? n1 : acc;
                acc = acc + wt[2] * x0;
                acc = round_bf4(acc, OUTF);
                sst4<kNtSt>(out, (long)off, OUTF, acc);
#pragma unroll
                for (int e = 0; e < 4; ++e) { const double a = (double)acc[e]; s1[e] += a; s2[e] = fma(a, a, s2[e]); }
            }
            x2 = x1;
            x1 = x0;
        }
    }
    // per-workgroup BatchNorm partial sums; a thread's channel quad is tid & 3 (as k_dw16)
#pragma unroll
    for (int e = 0; e < 4; ++e) { s1[e] = wave_sum_xor(s1[e], 4, 32); s2[e] = wave_sum_xor(s2[e], 4, 32); }
    if ((tid & 63) < 4)
#pragma unroll
        for (int e = 0; e < 4; ++e) { sStat[tid >> 6][4 * q + e] = s1[e]; sStat[tid >> 6][16 + 4 * q + e] = s2[e]; }
    __syncthreads();
    if (tid < 32) {
        double t = 0.0;
        for (int w2 = 0; w2 < NT / 64; ++w2) t += sStat[w2][tid];
        st_part(stat_partial + (long)blockIdx.x * 32 + tid, t, fa);
    }
    if (fa.kind) fin_reduce(stat_partial, 32, (int)blockIdx.x, gridDim.x, fa);
}

// ------------------------------------------------------------------------------ BatchNorm
// nn.BatchNorm2d in train mode (ConvBlock :159, GTConvBlock :190/:218/:222, TCN :269/:282/:286):
// biased batch variance for the normalisation, unbiased for the running estimate, momentum 0.1, eps 1e-5.
// Reductions: a thread walks the tensor with a stride that is a multiple of C, so it sees fixed
// channels; it accumulates a bounded number of elements in fp32, the per-thread sums are combined in
// double (workgroup, then across workgroups) in a fixed order.
template <int NV, int V, class TV>   // NV sums per channel, V channels per thread (vector width); TV float or double
__device__ __forceinline__ void block_reduce_store(const TV (&v)[NV][V], int C, double* sh, double* dst, bool pub) {
    const int tid = threadIdx.x, groups = C / V;      // threads with equal (tid % groups) share channels
    if ((groups & (groups - 1)) == 0 && groups <= 32) {
        // lanes first (xor shuffles over the lane bits above the channel group), then the NT/64 waves through LDS.
        // (The one-thread-per-channel loop over all NT entries below cost 64 dependent LDS reads per value: the
        // 12 values of the BatchNorm backward made a 40 us tail on a 95 us streaming pass.)
        const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            double r[V];
#pragma unroll
            for (int e = 0; e < V; ++e) r[e] = wave_sum_xor((double)v[k][e], groups, 32);
            __syncthreads();
            if (lane < groups)
#pragma unroll
                for (int e = 0; e < V; ++e) sh[wv * C + lane * V + e] = r[e];
            __syncthreads();
            if (tid < C) {
                double s = 0.0;
                for (int w = 0; w < NT / 64; ++w) s += sh[w * C + tid];
                if (pub) st_pub(dst + k * C + tid, s);
                else dst[k * C + tid] = s;
            }
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int e = 0; e < V; ++e) {
            __syncthreads();
            sh[tid] = (double)v[k][e];
            __syncthreads();
            if (tid < groups) {
                double s = 0.0;
                for (int i = tid; i < NT; i += groups) s += sh[i];
                if (pub) st_pub(dst + k * C + tid * V + e, s);
                else dst[k * C + tid * V + e] = s;
            }
        }
}

template <int V>
__global__ __launch_bounds__(NT) void k_bn_stats(const float* __restrict__ y, long total, int C,
                                                double* __restrict__ partial, int bf, FinArgs fa) {
    __shared__ double sh[NT];
    double v[2][V];    // double from the first addition on: no cancellation in E[y^2] - mean^2 (see k_conv_mfma)
#pragma unroll
    for (int e = 0; e < V; ++e) v[0][e] = v[1][e] = 0.0;
    const long units = total / V;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < units; i += (long)gridDim.x * NT) {
        float x[V];
        load_vec_s<V, kNt>(y, i * V, bf, x);
#pragma unroll
        for (int e = 0; e < V; ++e) { const double a = (double)x[e]; v[0][e] += a; v[1][e] = fma(a, a, v[1][e]); }
    }
    block_reduce_store<2, V>(v, C, sh, partial + (long)blockIdx.x * 2 * C, fa.kind != 0);
    if (fa.kind) fin_reduce(partial, 2 * C, blockIdx.x, gridDim.x, fa);
}

// sums the per-workgroup partials [nparts][K] (K <= 64 values) with 1024 threads: 64 values x 16 slices
__device__ __forceinline__ double reduce_partials(const double* partial, int nparts, int K, double (*sh)[64]) {
    const int j = threadIdx.x & 63, slice = threadIdx.x >> 6;
    double s = j < K ? sum_strided(partial + j, slice, nparts, 16, K) : 0.0;
    sh[slice][j] = s;
    __syncthreads();
    if (slice == 0)
        for (int q = 1; q < 16; ++q) s += sh[q][j];
    return s;    // valid in threads 0..K-1
}

__global__ __launch_bounds__(1024) void k_bn_stats_finish(const double* __restrict__ partial, int nparts, long n, int C,
                                                         float* __restrict__ stats, float* __restrict__ rmean,
                                                         float* __restrict__ rvar, float* __restrict__ shift,
                                                         float* __restrict__ stats_b) {
    // (the separate second stage: runs only with the in-launch finish switched off, fusion bit 10)
    __shared__ double sh[16][64];
    __shared__ double tot[64];
    const double s = reduce_partials(partial, nparts, 2 * C, sh);
    if (threadIdx.x < 2 * C) tot[threadIdx.x] = s;
    __syncthreads();
    bn_stats_math(tot, n, C, stats, rmean, rvar, shift, stats_b);
}

__device__ __forceinline__ float act_fwd(float z, int act, float slope) {
    if (act == ACT_PRELU) return z > 0.f ? z : slope * z;     // nn.PReLU(), one shared slope
    if (act == ACT_TANH) return tanhf(z);
    return z;
}

template <int V>
__global__ __launch_bounds__(NT) void k_bn_act(const float* __restrict__ y, long total, int C,
                                              const float* __restrict__ stats, const float* __restrict__ gamma,
                                              const float* __restrict__ beta, const float* __restrict__ res, int act,
                                              const float* __restrict__ slope, float* __restrict__ a, int bf, int ybf,
                                              float* __restrict__ a2, int a2_bf, float* __restrict__ y2, int y2_bf,
                                              const float* __restrict__ post) {
    const float sl = slope ? slope[0] : 0.f;
    const long units = total / V;
    // the stride is a multiple of C: the thread's channels and their constants are fixed
    const int c0 = (int)((((long)blockIdx.x * NT + threadIdx.x) * V) % C);
    float mean[V], istd[V], gm[V], bt[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { mean[e] = stats[c0 + e]; istd[e] = stats[C + c0 + e]; gm[e] = gamma[c0 + e]; bt[e] = beta[c0 + e]; }
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < units; i += (long)gridDim.x * NT) {
        float x[V], r[V], o[V], yt[V], pa[V];
        load_vec_s<V, kNt>(y, i * V, ybf, x);
        if (res) load_vec_s<V, kNt>(res, i * V, bf, r);
        if (post) load_vec_s<V, kNt>(post, i * V, bf, pa);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            // same expression order as the backward's recomputation of z: gamma * ((y - mean) * invstd) + beta
            float z = gm[e] * ((x[e] - mean[e]) * istd[e]) + bt[e];
            if (res) z += r[e];
            o[e] = act_fwd(z, act, sl);
            // post: the decoder's skip is added AFTER the activation and the sum is what gets stored (the next layer's
            // input x + skip; the activation itself has no other reader) -- the same fp32 add the separate pass made
            if (post) o[e] = round16(o[e], bf) + pa[e];      // (16-bit storage: the activation rounded as the stored one was)
            if (y2) yt[e] = ycopy_value(x[e], z, mean[e], istd[e], gm[e], bt[e], res != nullptr, res ? r[e] : 0.f, y2_bf,
                                        act == ACT_PRELU);
        }
        if (y2) {          // exact chain: the centred, kink-consistent 16-bit copy of y for the backward
            if constexpr (V == 4) sst4<kNtSt>(y2, i * 4, y2_bf, f32x4{yt[0], yt[1], yt[2], yt[3]});
            else sst1(y2, i, y2_bf, yt[0]);
        }
        if constexpr (V == 4) sst4<kNtSt>(a, i * 4, bf, f32x4{o[0], o[1], o[2], o[3]});
        else sst1(a, i, bf, o[0]);
        if (a2) {          // exact chain: the backward's 16-bit copy next to the fp32 value
            if constexpr (V == 4) sst4<kNtSt>(a2, i * 4, a2_bf, f32x4{o[0], o[1], o[2], o[3]});
            else sst1(a2, i, a2_bf, o[0]);
        }
    }
}

__device__ __forceinline__ float act_bwd(float z, float g, int act, float sl, float& dsl) {
    if (act == ACT_PRELU) { dsl = z > 0.f ? 0.f : g * z; return z > 0.f ? g : sl * g; }
    dsl = 0.f;
    if (act == ACT_TANH) { const float t = tanhf(z); return g * (1.f - t * t); }
    return g;
}

// backward, pass 1: S1 = sum dz, S2 = sum dz * xhat, S3 = sum da * min(z, 0) (PReLU slope gradient)
// FMT >= 0: the storage formats as a compile-time constant (FMT = bf * 4 + ybf): with the run-time flags every load sits
// behind its own wave-uniform branch, i.e. in its own basic block, and the U strides of loads below are issued one at
// a time after all (this read-only pass ran at 3.5 TB/s); FMT < 0: run-time flags (the odd channel counts).
// ACT >= 0: the activation as a compile-time constant too (with the run-time switch every ELEMENT went through four
// scalar branches: 64 taken branches per trip of a pass that should only wait for its loads)
template <int V, int FMT = -1, int ACT = -1, int GF = 0>      // GF: storage format of da (see k_unit1x1_bwd)
__global__ __launch_bounds__(NT) void k_bn_bwd_reduce(const float* __restrict__ da, const float* __restrict__ y,
                                                     long total, int C, const float* __restrict__ stats,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     const float* __restrict__ res, int act_rt,
                                                     const float* __restrict__ slope, double* __restrict__ partial,
                                                     int bf_rt, int ybf_rt, FinArgs fa) {
    const int bf = FMT >= 0 ? FMT / 4 : bf_rt, ybf = FMT >= 0 ? FMT % 4 : ybf_rt, act = ACT >= 0 ? ACT : act_rt;
    __shared__ double sh[NT];
    const float sl = slope ? slope[0] : 0.f;
    float v[3][V];
#pragma unroll
    for (int e = 0; e < V; ++e) v[0][e] = v[1][e] = v[2][e] = 0.f;
    const long units = total / V;
    const int c0 = (int)((((long)blockIdx.x * NT + threadIdx.x) * V) % C);   // fixed per thread
    float mean[V], istd[V], gm[V], bt[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { mean[e] = stats[c0 + e]; istd[e] = stats[C + c0 + e]; gm[e] = gamma[c0 + e]; bt[e] = beta[c0 + e]; }
    // U grid-strides per trip with all their loads issued first (a read-only pass has nothing but its own loads in
    // flight to cover the HBM latency: two 16-byte loads per thread ran at 3.5 TB/s); the sums are still taken in index
    // order, so the result is bit-identical to the one-stride loop
    constexpr int U = 4;
    const long stride = (long)gridDim.x * NT;
    for (long i0 = (long)blockIdx.x * NT + threadIdx.x; i0 < units; i0 += U * stride) {
        float x[U][V], g[U][V], r[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long i = i0 + u * stride < units ? i0 + u * stride : i0;     // clamped: a valid element, not summed
            load_vec_s<V, kNt>(y, i * V, ybf, x[u]);
            load_vec_s<V, kNt>(da, i * V, GF, g[u]);
            if (res) load_vec_s<V, kNt>(res, i * V, bf, r[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (i0 + u * stride >= units) break;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float xh = (x[u][e] - mean[e]) * istd[e];
                float z = gm[e] * xh + bt[e];
                if (res) z += r[u][e];
                float dsl;
                const float dz = act_bwd(z, g[u][e], act, sl, dsl);
                v[0][e] += dz;
                v[1][e] = fmaf(dz, xh, v[1][e]);
                v[2][e] += dsl;
            }
        }
    }
    block_reduce_store<3, V>(v, C, sh, partial + (long)blockIdx.x * 3 * C, fa.kind != 0);
    if (fa.kind) fin_reduce(partial, 3 * C, blockIdx.x, gridDim.x, fa);
}

__global__ __launch_bounds__(1024) void k_bn_bwd_finish(const double* __restrict__ partial, int nparts, long n, int C,
                                                       float* __restrict__ red, float* __restrict__ dgamma,
                                                       float* __restrict__ dbeta, float* __restrict__ dslope) {
    __shared__ double sh[16][64];
    __shared__ double tot[64];
    const double s = reduce_partials(partial, nparts, 3 * C, sh);
    if (threadIdx.x < 3 * C) tot[threadIdx.x] = s;
    __syncthreads();
    bn_bwd_math(tot, n, C, red, dgamma, dbeta, dslope);
}

// pass 2: dy = gamma * invstd * (dz - mean(dz) - xhat * mean(dz * xhat)); dres (+)= dz
template <int V>
__global__ __launch_bounds__(NT) void k_bn_bwd_apply(const float* __restrict__ da, const float* __restrict__ y,
                                                    long total, int C, const float* __restrict__ stats,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    const float* __restrict__ res, int act,
                                                    const float* __restrict__ slope, const float* __restrict__ red,
                                                    float* __restrict__ dy, float* __restrict__ dres, int dres_acc,
                                                    int bf, int ybf, int gbf) {
    const float sl = slope ? slope[0] : 0.f;
    const long units = total / V;
    const int c0 = (int)((((long)blockIdx.x * NT + threadIdx.x) * V) % C);
    float mean[V], istd[V], gm[V], bt[V], m1[V], m2[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        mean[e] = stats[c0 + e]; istd[e] = stats[C + c0 + e]; gm[e] = gamma[c0 + e]; bt[e] = beta[c0 + e];
        m1[e] = red[c0 + e]; m2[e] = red[C + c0 + e];
    }
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < units; i += (long)gridDim.x * NT) {
        float x[V], g[V], r[V], o[V], dzv[V];
        load_vec_s<V, kNt>(y, i * V, ybf, x);
        load_vec_s<V, kNt>(da, i * V, gbf, g);
        if (res) load_vec_s<V, kNt>(res, i * V, bf, r);
        if (dres && dres_acc) load_vec_s<V, kNt>(dres, i * V, gbf, dzv);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float xh = (x[e] - mean[e]) * istd[e];
            float z = gm[e] * xh + bt[e];
            if (res) z += r[e];
            float dsl;
            const float dz = act_bwd(z, g[e], act, sl, dsl);
            dzv[e] = (dres && dres_acc) ? dzv[e] + dz : dz;
            o[e] = gm[e] * istd[e] * (dz - m1[e] - xh * m2[e]);
        }
        if constexpr (V == 4) {
            *reinterpret_cast<f32x4*>(dy + i * 4) = f32x4{o[0], o[1], o[2], o[3]};     // (dy: this unit's own scratch, fp32)
            if (dres) sst4(dres, i * 4, gbf, f32x4{dzv[0], dzv[1], dzv[2], dzv[3]});
        } else {
            dy[i] = o[0];
            if (dres) sst1(dres, i, gbf, dzv[0]);
        }
    }
}

// depthwise weight gradient, C = 16, streaming form: a thread owns 4 channels and walks the positions with a
// stride that keeps them fixed; dW[c][tap] = sum_pos dout[pos][c] * in[pos + tap][c] and db = sum dout are
// per-thread fp32 partial sums, combined in double in a fixed order (workgroup, then k_dw_wgrad_finish2).
template <int NKT, int NKF, int FIN = -1>     // FIN: storage format of `in`, compile time (see k_dw16)
__global__ __launch_bounds__(NT) void k_dw_wgrad_stream(DwGeom g, const float* __restrict__ in,
                                                       const float* __restrict__ dout, double* __restrict__ partial,
                                                       StrideIter it) {
    const unsigned vb = xcd_block();
    constexpr int NTAP = NKT * NKF;
    __shared__ double sh[NT];
    float v[NTAP + 1][4];
#pragma unroll
    for (int k = 0; k <= NTAP; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[k][e] = 0.f;
    const long units = (long)g.B * g.Tout * g.F * 4;
    const int q = threadIdx.x & 3;
    RowPos P;
    P.init(((long)vb * NT + threadIdx.x) >> 2, g.F, g.Tout);
    for (long i = (long)vb * NT + threadIdx.x; i < units; i += (long)gridDim.x * NT) {
        const long p = i >> 2;
        const f32x4 d = *reinterpret_cast<const f32x4*>(dout + p * 16 + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[NTAP][e] += d[e];
        // all tap loads first (a tap outside the tensor loads the centre record and contributes d * 0), as in k_dw16
        constexpr int FR = FIN < 0 ? 0 : FIN;
        f32x4 xv[NTAP];
        typename Raw4<FR>::t xr[NTAP];
        bool okv[NTAP];
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int kf = 0; kf < NKF; ++kf) {
                const int ti = P.to + g.t_off[kt], fi = P.fo + g.f_off[kf];
                const bool ok = ti >= 0 && ti < g.Tin && fi >= 0 && fi < g.F;
                const long rec = ok ? (long)(P.bt + g.t_off[kt]) * g.F + fi : p;
                okv[kt * NKF + kf] = ok;
                if constexpr (FIN < 0) xv[kt * NKF + kf] = sld4(in, rec * 16 + 4 * q, g.in_bf);     // (no use of the value in this loop)
                else xr[kt * NKF + kf] = sld4_raw<FR>(in, rec * 16 + 4 * q);
            }
        if constexpr (FIN >= 0) {
#pragma unroll
            for (int tp = 0; tp < NTAP; ++tp) xv[tp] = dec4<FR>(xr[tp]);
        }
#pragma unroll
        for (int tp = 0; tp < NTAP; ++tp)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[tp][e] = fmaf(d[e], okv[tp] ? xv[tp][e] : 0.f, v[tp][e]);
        P.advance(it, g.F, g.Tout);
    }
    block_reduce_store<NTAP + 1, 4>(v, 16, sh, partial + (long)vb * (NTAP + 1) * 16);
}
// partial [nparts][(ntap+1)*16] (tap-major, bias last) -> dw, dbias; grid = ceil(K / 64) workgroups of 1024
__global__ __launch_bounds__(1024) void k_dw_wgrad_finish2(DwGeom g, const double* __restrict__ partial, int nparts,
                                                          float* __restrict__ dw, float* __restrict__ dbias) {
    __shared__ double sh[16][64];
    const int ntap = g.nkt * g.nkf, K = (ntap + 1) * 16;
    const int j = threadIdx.x & 63, slice = threadIdx.x >> 6, k = blockIdx.x * 64 + j;
    double s = k < K ? sum_strided(partial + k, slice, nparts, 16, K) : 0.0;
    sh[slice][j] = s;
    __syncthreads();
    if (slice != 0 || k >= K) return;
    for (int q = 1; q < 16; ++q) s += sh[q][j];
    const int tap = k >> 4, c = k & 15;
    if (tap == ntap) {
        if (dbias) dbias[c] = (float)s;
    } else {
        const int kt = tap / g.nkf, kf = tap - kt * g.nkf;
        dw[c * g.w_c + kt * g.w_kt + kf * g.w_kf] = (float)s;
    }
}

// The weight-gradient finishes of a backward pass, BATCHED (fusion bit 15): the fused backward kernels leave per-workgroup
// partial sums, and 44 one-to-five-workgroup launches of k_wgrad_mfma_finish / k_dw_wgrad_finish2 per step (6-7 us each,
// ~0.3 ms, each behind a kernel boundary of the main stream) added them up.  With the bit on every unit's partials go to
// a region of their own in a pool and the launcher only RECORDS the finish; gtcrn_train_backward runs them all in two
// launches at its end.  Same sums in the same order (sum_strided over the workgroups, 16 slices): bit-identical gradients.
struct WFin {
    const void* partial;       // float [nparts][K] (type 0) or double [nparts][K] (type 1)
    float* dw;
    float* dbias;
    int nparts, K, type;       // type 0: conv, K = ntap * 256 + 16; type 1: depthwise, K = (ntap + 1) * 16
    int ntap, nkf, Cout, Cin;
    int s0, s1, s2, s3;        // conv: w_co, w_ci, w_kt, w_kf; depthwise: w_c, w_kt, w_kf
};
constexpr int WFIN_BATCH = 24;
struct WFinBatch {
    int n;
    WFin e[WFIN_BATCH];
};
__global__ __launch_bounds__(1024) void k_wgrad_finish_batch(WFinBatch b) {
    __shared__ double sh[16][64];
    const WFin& f = b.e[blockIdx.y];
    const int K = f.K;
    if ((int)blockIdx.x * 64 >= K) return;                         // (uniform: this entry has fewer columns)
    const int j = threadIdx.x & 63, slice = threadIdx.x >> 6, k = blockIdx.x * 64 + j;
    double s = 0.0;
    if (k < K) {
        if (f.type == 0) s = sum_strided(reinterpret_cast<const float*>(f.partial) + k, slice, f.nparts, 16, K);
        else s = sum_strided(reinterpret_cast<const double*>(f.partial) + k, slice, f.nparts, 16, K);
    }
    sh[slice][j] = s;
    __syncthreads();
    if (slice != 0 || k >= K) return;
    for (int q = 1; q < 16; ++q) s += sh[q][j];
    if (f.type == 0) {
        if (k >= f.ntap * 256) {
            const int co = k - f.ntap * 256;
            if (f.dbias && co < f.Cout) f.dbias[co] = (float)s;
        } else {
            const int tap = k >> 8, co = (k >> 4) & 15, ci = k & 15, kt = tap / f.nkf, kf = tap - kt * f.nkf;
            if (co < f.Cout && ci < f.Cin) f.dw[co * f.s0 + ci * f.s1 + kt * f.s2 + kf * f.s3] = (float)s;
        }
    } else {
        const int tap = k >> 4, c = k & 15;
        if (tap == f.ntap) {
            if (f.dbias) f.dbias[c] = (float)s;
        } else {
            const int kt = tap / f.nkf, kf = tap - kt * f.nkf;
            f.dw[c * f.s0 + kt * f.s1 + kf * f.s2] = (float)s;
        }
    }
}
// SFE_Lite weight gradient (3 channels, (1,3) taps, no bias): one thread per position, all 3 channels
__global__ __launch_bounds__(NT) void k_sfe_wgrad(const float* __restrict__ in, const float* __restrict__ dout, long rows,
                                                 int F, double* __restrict__ partial, int bf) {
    __shared__ double sh[NT];
    float v[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int e = 0; e < 3; ++e) v[k][e] = 0.f;
    const long npos = rows * F;
    for (long p = (long)blockIdx.x * NT + threadIdx.x; p < npos; p += (long)gridDim.x * NT) {
        const int f = (int)(p % F);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int fi = f + k - 1;
            if (fi < 0 || fi >= F) continue;
#pragma unroll
            for (int e = 0; e < 3; ++e) v[k][e] = fmaf(dout[p * 3 + e], sld1(in, (p + k - 1) * 3 + e, bf), v[k][e]);
        }
    }
    block_reduce_store<3, 3>(v, 3, sh, partial + (long)blockIdx.x * 9);
}
__global__ __launch_bounds__(1024) void k_sfe_wgrad_finish(const double* __restrict__ partial, int nparts,
                                                          float* __restrict__ dw) {
    __shared__ double sh[16][64];
    const double s = reduce_partials(partial, nparts, 9, sh);
    const int k = threadIdx.x;                 // partial order [tap][c]; weight layout [c][1][1][tap]
    if (k < 9) dw[(k % 3) * 3 + k / 3] = (float)s;
}

// generic: out[k] = sum over workgroups of float partials [nparts][K]; grid = ceil(K / 64) x 1024 threads
__global__ __launch_bounds__(1024) void k_reduce_partials_f(const float* __restrict__ partial, int nparts, int K,
                                                           float* __restrict__ out) {
    __shared__ double sh[16][64];
    const int j = threadIdx.x & 63, slice = threadIdx.x >> 6, k = blockIdx.x * 64 + j;
    double s = k < K ? sum_strided(partial + k, slice, nparts, 16, K) : 0.0;
    sh[slice][j] = s;
    __syncthreads();
    if (slice != 0 || k >= K) return;
    for (int q = 1; q < 16; ++q) s += sh[q][j];
    out[k] = (float)s;
}

// ------------------------------------------------------ fused backward of a 1x1 conv + BatchNorm + activation
// For the 28 pointwise units (point_conv1/2 of the GTConv blocks, conv1/conv3 of the TCN blocks) the three
// backward passes after the reduction -- BatchNorm/activation backward (dy), data gradient (dx = W^T dy) and
// weight gradient (dW = sum_pos dy x^T) -- run in ONE pass over a tile of 16 positions:
//   lane (n, q) loads da and y of position n, channels 4q..4q+3, forms dz and dy in registers (dres = dz is
//   stored for the residual of a TCN block), feeds dy straight into the data-gradient MFMAs as the B operand,
//   and parks the dy tile in a wave-private LDS tile from which the weight-gradient MFMAs read it back with
//   positions as the K index (lane (c, k) = channel c of position 4u + k), next to x loaded in that layout.
// Replaces k_bn_bwd_apply + k_conv_wgrad_mfma<1,1> + k_conv_mfma<1,1>: 4 tensor passes instead of 7.
struct BnBwdArgs {
    const float *stats, *gamma, *beta, *slope, *red;
    int act;
};
// NEXT: see NextRedArgs; rpartial [gridDim.x][48] doubles
// GF: storage format of the GRADIENT tensors handed between units (da, dx, dres): 0 fp32, 1 bf16 (storage mode 5: the
// inter-unit gradients of the bf16 mode are rounded to bf16 where a unit stores them -- what autocast-style training does --
// which halves the remaining fp32 streams of that mode; arithmetic, reductions and parameter gradients stay fp32)
template <int FMT, int YF, bool NEXT = false, bool XR = false, int GF = 0>   // storage formats of x / res and of y, compile time (see sld1)
__global__ __launch_bounds__(NT) void k_unit1x1_bwd(ConvGeom g, const float* __restrict__ x, const float* __restrict__ y,
                                                   const float* __restrict__ da, const float* __restrict__ res,
                                                   BnBwdArgs bn, const float* __restrict__ w,
                                                   float* __restrict__ dx, int dx_acc, float* __restrict__ dres,
                                                   int dres_acc, float* __restrict__ partial, long tiles_per_wave,
                                                   NextRedArgs nx, double* __restrict__ rpartial, FinArgs fa) {
    __shared__ double sRed[NEXT ? NT / 64 : 1][48];
    f32x4 nmean = {0, 0, 0, 0}, nistd = nmean, ngm = nmean, nbt = nmean;
    float nsl = 0.f, vr[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) vr[0][e] = vr[1][e] = vr[2][e] = 0.f;
    if constexpr (NEXT) {
        const int q4 = 4 * ((threadIdx.x & 63) >> 4);
        nmean = *reinterpret_cast<const f32x4*>(nx.stats + q4); nistd = *reinterpret_cast<const f32x4*>(nx.stats + 16 + q4);
        ngm = *reinterpret_cast<const f32x4*>(nx.gamma + q4); nbt = *reinterpret_cast<const f32x4*>(nx.beta + q4);
        nsl = nx.slope[0];
    }
    __shared__ __attribute__((aligned(16))) float sWt[256];        // data-gradient A matrix [ci][co] = W[co][ci]
    __shared__ __attribute__((aligned(16))) float sT[NT / 64][256];   // per wave: dy tile [pos][16]
    __shared__ __attribute__((aligned(16))) float sX[NT / 64][256];   // per wave: the x tile [pos][16] (loaded, or XR: recomputed)
    static_assert(!XR || NEXT, "x is recomputed from the NEXT unit's y");
    __shared__ float sAcc[NT / 64][256 + 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 15, q = lane >> 4;
    {
        const int ci = tid >> 4, co = tid & 15;
        sWt[tid] = (co < g.Cout && ci < g.Cin) ? w[co * g.w_co + ci * g.w_ci] : 0.f;
    }
    __syncthreads();
    const long npos = (long)g.B * g.Tout * g.Fout, ntiles = (npos + 15) >> 4;
    const long wave = (long)blockIdx.x * (NT / 64) + wv;
    long tile = wave * tiles_per_wave;
    const long tend = tile + tiles_per_wave < ntiles ? tile + tiles_per_wave : ntiles;
    const bool co_ok4 = 4 * q < g.Cout, ci_ok4 = 4 * q < g.Cin;
    const int c = n, k = q;                                         // (c, k) role of the lane in the weight gradient
    const bool co_ok = c < g.Cout, ci_ok = c < g.Cin;
    const float sl = bn.slope ? bn.slope[0] : 0.f;
    f32x4 mean = {0, 0, 0, 0}, istd = mean, gm = mean, bt = mean, m1 = mean, m2 = mean;
    if (co_ok4) {
        mean = *reinterpret_cast<const f32x4*>(bn.stats + 4 * q);
        istd = *reinterpret_cast<const f32x4*>(bn.stats + g.Cout + 4 * q);
        gm = *reinterpret_cast<const f32x4*>(bn.gamma + 4 * q);
        bt = *reinterpret_cast<const f32x4*>(bn.beta + 4 * q);
        m1 = *reinterpret_cast<const f32x4*>(bn.red + 4 * q);
        m2 = *reinterpret_cast<const f32x4*>(bn.red + g.Cout + 4 * q);
    }
    const f32x4 At = *reinterpret_cast<const f32x4*>(sWt + n * 16 + 4 * q);   // row ci = n of W^T
    f32x4 accW = {0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    // Round 5 (late): the loop below is issue-bound once the tensors are 16-bit (180 us on 0.8 GB), so it is written for
    // instruction count -- quad-wide expressions (packed fp32 instructions), 32-bit lane offsets from wave-uniform bases
    // advanced per tile, the activation derivative as one select (PReLU, or "none" as slope 1: the pointwise units have
    // no other activation, the launcher checks).
    const float slw = bn.act == ACT_PRELU ? sl : 1.f;
    const f32x4 gi = gm * istd;
    f32x4 vrv[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const int np32 = (int)npos;                                       // (positions and element offsets fit in 31 bits: the launcher checks)
    int p = (int)(tile * 16) + n;
    unsigned yoff = (unsigned)p * (unsigned)g.Cout + 4u * q;          // y, da, res, dres: [pos][Cout]
    unsigned xoff = (unsigned)p * (unsigned)g.CinT + (unsigned)g.cin_off + 4u * q;   // x, dx (and, NEXT: that unit's y / res)
    const unsigned ystep = 16u * (unsigned)g.Cout, xstep = 16u * (unsigned)g.CinT;
    struct TileIn {
        typename Raw4<YF>::t y, ny;
        typename Raw4<GF>::t da;
        typename Raw4<FMT>::t x, r, nr;
    };
    auto fetch = [&](int pp, unsigned yo, unsigned xo, TileIn& ti) {
        const bool pvv = pp < np32;
        const unsigned yq = (pvv && co_ok4) ? yo : 0u, xq = (pvv && ci_ok4) ? xo : 0u;
        ti.y = sld4_raw<YF, kNt>(y, (long)yq);
        ti.da = sld4_raw<GF, kNt>(da, (long)yq);
        if (res) ti.r = sld4_raw<FMT, kNt>(res, (long)yq);
        if constexpr (!XR) ti.x = sld4_raw<FMT, true>(x, (long)xq);
        if constexpr (NEXT) {
            ti.ny = sld4_raw<YF, kNt>(nx.y, (long)(pvv ? xo : 0u));
            if (nx.res) ti.nr = sld4_raw<FMT, kNt>(nx.res, (long)(pvv ? xo : 0u));
        }
    };
    // (requesting tile i + 1's loads before tile i is computed -- what pays in k_pw_fwd -- made this kernel SLOWER: the bf16
    // step 22.27 ms with it against 21.79 without, same box; its registers also cost the fp32 form a wave per SIMD)
    TileIn cur{};
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    for (; tile < tend; ++tile) {
        const bool pv = p < np32;
        fetch(p, yoff, xoff, cur);
        f32x4 nxh = zero4, nz = zero4;                             // the NEXT unit's xhat and pre-activation z of this lane's quad
        if constexpr (NEXT) {      // (Cin == CinT == 16 with NEXT: the launcher checks)
            nxh = (dec4<YF>(cur.ny) - nmean) * nistd;
            nz = ngm * nxh + nbt;
            if (nx.res) nz += dec4<FMT>(cur.nr);
            if constexpr (XR) {    // x = PReLU(z), the expressions of pre_apply / k_bn_act
                f32x4 xa;
#pragma unroll
                for (int e = 0; e < 4; ++e) xa[e] = nz[e] > 0.f ? nz[e] : nsl * nz[e];
                if (nx.xround) xa = round_bf4(xa, 1);
                *reinterpret_cast<f32x4*>(&sX[wv][n * 16 + 4 * q]) = pv ? xa : zero4;
            }
        }
        if constexpr (!XR) *reinterpret_cast<f32x4*>(&sX[wv][n * 16 + 4 * q]) = (pv && ci_ok4) ? dec4<FMT>(cur.x) : zero4;
        f32x4 dy = zero4;
        {
            const f32x4 xh = (dec4<YF>(cur.y) - mean) * istd;
            f32x4 z = gm * xh + bt;
            if (res) z += dec4<FMT>(cur.r);
            const f32x4 gv = dec4<GF>(cur.da), gs = slw * gv;
            f32x4 dzv;
#pragma unroll
            for (int e = 0; e < 4; ++e) dzv[e] = z[e] > 0.f ? gv[e] : gs[e];
            const f32x4 dyv = gi * (dzv - m1 - xh * m2);
            if (pv && co_ok4) {
                dy = dyv;
                if (dres) {
                    if (dres_acc) sst4(dres, (long)yoff, GF, sld4(dres, (long)yoff, GF) + dzv);
                    else sst4<kNtSt>(dres, (long)yoff, GF, dzv);
                }
            }
        }
        // data gradient: dx[pos][ci] = sum_co W[co][ci] dy[pos][co]
        if (dx) {
            f32x4 acc = zero4;
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = mfma4(At[e], dy[e], acc);
            if (pv && ci_ok4) {
                if (dx_acc) acc = sld4(dx, (long)xoff, GF) + acc;
                acc = round_bf4(acc, GF);          // (the riding reduction below sees the value the tensor now holds)
                if (dx_acc) sst4(dx, (long)xoff, GF, acc);
                else sst4<kNtSt>(dx, (long)xoff, GF, acc);
                if constexpr (NEXT) {
                    const f32x4 as = nsl * acc, az = acc * nz;
                    f32x4 dz2, ds2;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool pos = nz[e] > 0.f;
                        dz2[e] = pos ? acc[e] : as[e];
                        ds2[e] = pos ? 0.f : az[e];
                    }
                    vrv[0] += dz2;
                    vrv[1] += dz2 * nxh;
                    vrv[2] += ds2;
                }
            }
        }
        // weight gradient: dy tile through wave-private LDS into the (c, k) layout
        *reinterpret_cast<f32x4*>(&sT[wv][n * 16 + 4 * q]) = dy;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float a = sT[wv][(4 * u + k) * 16 + c];
            bsum += a;
            accW = mfma4(a, sX[wv][(4 * u + k) * 16 + c], accW);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        p += 16;
        yoff += ystep;
        xoff += xstep;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { vr[0][e] = vrv[0][e]; vr[1][e] = vrv[1][e]; vr[2][e] = vrv[2][e]; }
    (void)co_ok; (void)ci_ok;
    // per-workgroup partial dW / db, same layout as k_conv_wgrad_mfma<1,1>: [co*16 + ci] then 16 bias sums
#pragma unroll
    for (int r = 0; r < 4; ++r) sAcc[wv][(4 * k + r) * 16 + c] = accW[r];
    sAcc[wv][256 + lane] = bsum;
    __syncthreads();
    float* pp = partial + (long)blockIdx.x * (256 + 16);
    {
        float t = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < NT / 64; ++w2) t += sAcc[w2][tid];
        pp[tid] = t;
    }
    if (tid < 16) {
        float t = 0.f;
        for (int w2 = 0; w2 < NT / 64; ++w2)
            for (int kk = 0; kk < 4; ++kk) t += sAcc[w2][256 + kk * 16 + tid];
        pp[256 + tid] = t;
    }
    if constexpr (NEXT) {
        // lanes of one channel quad differ in n (xor distances 8..1), then the waves through LDS
#pragma unroll
        for (int k3 = 0; k3 < 3; ++k3)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double t = wave_sum_xor((double)vr[k3][e], 1, 8);
                if (n == 0) sRed[wv][k3 * 16 + 4 * q + e] = t;
            }
        __syncthreads();
        if (tid < 48) {
            double t = 0.0;
            for (int w2 = 0; w2 < NT / 64; ++w2) t += sRed[w2][tid];
            st_part(rpartial + (long)blockIdx.x * 48 + tid, t, fa);
        }
        if (fa.kind) fin_reduce(rpartial, 48, blockIdx.x, gridDim.x, fa);
    }
}

// ------------------------------------------ fused backward of a depthwise (3,1) conv + BatchNorm + PReLU (TCN conv2)
// After the BatchNorm reduction the three remaining passes of such a unit -- dy = BatchNorm/PReLU backward
// (k_bn_bwd_apply: read da, y, write dy), the weight gradient (k_dw_wgrad_stream: read dy, x at three frames) and the
// data gradient (k_dw16 on the adjoint taps: read dy at three frames, write dx) -- are ONE pass: thread (position,
// channel quad) forms dy at its own frame t and at t + d, t + 2d (the frames its dx needs; da and y of those come from
// the L2), multiplies dy(t) with x(t - 2d), x(t - d), x(t) for the weight gradient and writes dx; dy never exists in
// memory.  Same per-element expressions as the separate kernels.  NEXT: the unit in FRONT (conv1) takes this dx as its
// da, so its own first backward pass (sum dz, sum dz * xhat, sum of the slope terms) is accumulated right here from
// one more read (its y) instead of a pass that re-reads dx and y.
// XR (with NEXT): x IS that unit's activation and is recomputed from its y at the three tap frames (see NextRedArgs).
template <int FX, int FY, bool NEXT, bool XR = false, int GF = 0>   // storage formats of x (an activation), of y / the next unit's y (conv outputs), of da / dx
__global__ __launch_bounds__(NT) void k_dwunit31_bwd(DwGeom g, const float* __restrict__ x, const float* __restrict__ y,
                                                    const float* __restrict__ da, BnBwdArgs bn,
                                                    const float* __restrict__ w, float* __restrict__ dx,
                                                    double* __restrict__ wpartial, NextRedArgs nx,
                                                    double* __restrict__ rpartial, StrideIter it, FinArgs fa) {
    const unsigned vb = xcd_block();
    __shared__ double sh[NT];
    const int tid = threadIdx.x, q = tid & 3;
    const f32x4 mean = *reinterpret_cast<const f32x4*>(bn.stats + 4 * q), istd = *reinterpret_cast<const f32x4*>(bn.stats + 16 + 4 * q);
    const f32x4 gm = *reinterpret_cast<const f32x4*>(bn.gamma + 4 * q), bt = *reinterpret_cast<const f32x4*>(bn.beta + 4 * q);
    const f32x4 m1 = *reinterpret_cast<const f32x4*>(bn.red + 4 * q), m2 = *reinterpret_cast<const f32x4*>(bn.red + 16 + 4 * q);
    const float sl = bn.slope[0];
    f32x4 wk[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) wk[k][e] = w[(4 * q + e) * g.w_c + k * g.w_kt];
    f32x4 nmean = {0, 0, 0, 0}, nistd = nmean, ngm = nmean, nbt = nmean;
    float nsl = 0.f;
    if constexpr (NEXT) {
        nmean = *reinterpret_cast<const f32x4*>(nx.stats + 4 * q); nistd = *reinterpret_cast<const f32x4*>(nx.stats + 16 + 4 * q);
        ngm = *reinterpret_cast<const f32x4*>(nx.gamma + 4 * q); nbt = *reinterpret_cast<const f32x4*>(nx.beta + 4 * q);
        nsl = nx.slope[0];
    }
    float vw[4][4], vr[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { vw[0][e] = vw[1][e] = vw[2][e] = vw[3][e] = 0.f; vr[0][e] = vr[1][e] = vr[2][e] = 0.f; }
    const int d1 = -g.t_off[1], d2 = -g.t_off[0];            // taps at t - 2d, t - d, t
    const long units = (long)g.B * g.Tout * g.F * 4;
    RowPos P;
    P.init(((long)vb * NT + tid) >> 2, g.F, g.Tout);
    for (long i = (long)vb * NT + tid; i < units; i += (long)gridDim.x * NT) {
        const long p = i >> 2;
        const bool f1 = P.to + d1 < g.Tout, f2 = P.to + d2 < g.Tout;     // frames t + d, t + 2d exist
        const bool b1 = P.to - d1 >= 0, b2 = P.to - d2 >= 0;             // frames t - d, t - 2d exist
        const long rf[3] = {p, f1 ? p + (long)d1 * g.F : p, f2 ? p + (long)d2 * g.F : p};
        const long rb[3] = {b2 ? p - (long)d2 * g.F : p, b1 ? p - (long)d1 * g.F : p, p};
        typename Raw4<FY>::t yr[3], ynr{}, ybr[2] = {};
        typename Raw4<FX>::t xr[3] = {};
        typename Raw4<GF>::t grr[3];
        f32x4 gr[3];
        static_assert(!XR || NEXT, "x is recomputed from the NEXT unit's y");
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            yr[j] = sld4_raw<FY>(y, rf[j] * 16 + 4 * q);
            grr[j] = sld4_raw<GF>(da, rf[j] * 16 + 4 * q);
            if constexpr (!XR) xr[j] = sld4_raw<FX>(x, rb[j] * 16 + 4 * q);
            else if (j < 2) ybr[j] = sld4_raw<FY>(nx.y, rb[j] * 16 + 4 * q);
        }
        if constexpr (NEXT) ynr = sld4_raw<FY>(nx.y, p * 16 + 4 * q);
        f32x4 dyv[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const f32x4 yv = dec4<FY>(yr[j]);
            gr[j] = dec4<GF>(grr[j]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xh = (yv[e] - mean[e]) * istd[e];
                const float z = gm[e] * xh + bt[e];
                const float dz = z > 0.f ? gr[j][e] : sl * gr[j][e];
                dyv[j][e] = gm[e] * istd[e] * (dz - m1[e] - xh * m2[e]);
            }
        }
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        dyv[1] = f1 ? dyv[1] : zero;
        dyv[2] = f2 ? dyv[2] : zero;
        f32x4 x0, x1, x2;
        if constexpr (XR) {
            auto xact = [&](const f32x4 yv) {        // PReLU(BatchNorm(y)) of the unit in front, as pre_apply forms it
                f32x4 a;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float z = ngm[e] * ((yv[e] - nmean[e]) * nistd[e]) + nbt[e];
                    const float v = z > 0.f ? z : nsl * z;
                    a[e] = nx.xround ? round16(v, 1) : v;
                }
                return a;
            };
            x0 = b2 ? xact(dec4<FY>(ybr[0])) : zero;
            x1 = b1 ? xact(dec4<FY>(ybr[1])) : zero;
            x2 = xact(dec4<FY>(ynr));
        } else {
            x0 = b2 ? dec4<FX>(xr[0]) : zero; x1 = b1 ? dec4<FX>(xr[1]) : zero; x2 = dec4<FX>(xr[2]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            vw[0][e] = fmaf(dyv[0][e], x0[e], vw[0][e]);
            vw[1][e] = fmaf(dyv[0][e], x1[e], vw[1][e]);
            vw[2][e] = fmaf(dyv[0][e], x2[e], vw[2][e]);
            vw[3][e] += dyv[0][e];
        }
        // dx(t) = w[0] dy(t + 2d) + w[1] dy(t + d) + w[2] dy(t): the adjoint taps in the order of k_dw16
        f32x4 acc = zero;
        acc = acc + wk[0] * dyv[2];
        acc = acc + wk[1] * dyv[1];
        acc = acc + wk[2] * dyv[0];
        acc = round_bf4(acc, GF);
        sst4<kNtSt>(dx, p * 16 + 4 * q, GF, acc);
        if constexpr (NEXT) {
            const f32x4 yn = dec4<FY>(ynr);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xh = (yn[e] - nmean[e]) * nistd[e];
                const float z = ngm[e] * xh + nbt[e];
                float dsl;
                const float dz = act_bwd(z, acc[e], ACT_PRELU, nsl, dsl);
                vr[0][e] += dz;
                vr[1][e] = fmaf(dz, xh, vr[1][e]);
                vr[2][e] += dsl;
            }
        }
        P.advance(it, g.F, g.Tout);
    }
    block_reduce_store<4, 4>(vw, 16, sh, wpartial + (long)vb * 64);
    if constexpr (NEXT) {
        block_reduce_store<3, 4>(vr, 16, sh, rpartial + (long)vb * 48, fa.kind != 0);
        if (fa.kind) fin_reduce(rpartial, 48, (int)vb, gridDim.x, fa);
    }
}

// The same unit's backward in the COLUMN form of k_dw31_col (fusion bit 14): k_dwunit31_bwd gives a thread one position and
// has it form dy at t, t + d, t + 2d and -- recomputing form -- the input activation at t - 2d, t - d, t: every dy and
// every activation of the tensor is computed three times, from nine to ten loads per thread.  A thread that walks ONE
// residue class of frames modulo the dilation computes each once and keeps three-deep windows: at step k it has dy_k
// and x_k and emits, for the element two steps back, the weight-gradient products dy_m (x_m-2, x_m-1, x_m), the data
// gradient dx_m = w0 dy_m+2 + w1 dy_m+1 + w2 dy_m (the adjoint taps in k_dw16's order) and the riding reduction of
// the unit in front.  A chunk of J outputs re-reads two elements on either side; all 3 (J + 2) loads of a chunk are
// requested before the first is used.  Same per-element expressions as k_dwunit31_bwd; sums in another order.
template <int F, int GF> struct DcBwdChunk { static constexpr int J = (F && GF) ? 8 : 4; };
template <int F, int GF, bool XR>      // F: storage format of x / y / the front unit's y; GF: of da / dx; XR: x recomputed
__global__ __launch_bounds__(NT) void k_dwunit31_col(int B, int T, int Fb, int d, int w_c, int w_kt, const float* __restrict__ x,
                                                    const float* __restrict__ y, const float* __restrict__ da, BnBwdArgs bn,
                                                    const float* __restrict__ w, float* __restrict__ dx,
                                                    double* __restrict__ wpartial, NextRedArgs nx,
                                                    double* __restrict__ rpartial, FinArgs fa) {
    constexpr int J = DcBwdChunk<F, GF>::J;
    __shared__ double sh[NT];
    const int tid = threadIdx.x, q = tid & 3;
    const f32x4 mean = *reinterpret_cast<const f32x4*>(bn.stats + 4 * q), istd = *reinterpret_cast<const f32x4*>(bn.stats + 16 + 4 * q);
    const f32x4 gm = *reinterpret_cast<const f32x4*>(bn.gamma + 4 * q), bt = *reinterpret_cast<const f32x4*>(bn.beta + 4 * q);
    const f32x4 m1 = *reinterpret_cast<const f32x4*>(bn.red + 4 * q), m2 = *reinterpret_cast<const f32x4*>(bn.red + 16 + 4 * q);
    const f32x4 gi = gm * istd;
    const float sl = bn.slope[0];
    f32x4 wk[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) wk[k][e] = w[(4 * q + e) * w_c + k * w_kt];
    const f32x4 nmean = *reinterpret_cast<const f32x4*>(nx.stats + 4 * q), nistd = *reinterpret_cast<const f32x4*>(nx.stats + 16 + 4 * q);
    const f32x4 ngm = *reinterpret_cast<const f32x4*>(nx.gamma + 4 * q), nbt = *reinterpret_cast<const f32x4*>(nx.beta + 4 * q);
    const float nsl = nx.slope[0];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 vwv[4] = {zero, zero, zero, zero}, vrv[3] = {zero, zero, zero};
    const int F4 = Fb * 4, S = ((T + d - 1) / d + J - 1) / J;
    const long items = (long)B * d * S * F4;
    const unsigned rowstep = (unsigned)d * (unsigned)Fb * 16u;
    for (long item = (long)blockIdx.x * NT + tid; item < items; item += (long)gridDim.x * NT) {
        const int fq = (int)(item % F4);
        long rest = item / F4;
        const int sc = (int)(rest % S);
        rest /= S;
        const int r = (int)(rest % d), b = (int)(rest / d);
        const int t0 = r + sc * J * d;
        if (t0 >= T) continue;
        const unsigned off0 = (unsigned)(((long)b * T + t0) * Fb * 16 + fq * 4);     // element (b, t0, f, 4q); < 2^31
        // step k: forward element j0 + k (da, y: frame t0 + k d) and backward element j0 - 2 + k (the front unit's y,
        // or x: frame t0 + (k - 2) d)
        typename Raw4<GF>::t gr[J + 2];
        typename Raw4<F>::t yr[J + 2], br[J + 2];
#pragma unroll
        for (int k = 0; k < J + 2; ++k) {
            const int tf = t0 + k * d, tb = t0 + (k - 2) * d;
            const unsigned of = tf < T ? off0 + (unsigned)k * rowstep : off0;
            const unsigned ob = (tb >= 0 && tb < T) ? off0 + (unsigned)(k - 2) * rowstep : off0;
            gr[k] = sld4_raw<GF, kNt>(da, (long)of);
            yr[k] = sld4_raw<F>(y, (long)of);
            br[k] = sld4_raw<F>(XR ? nx.y : x, (long)ob);
        }
        typename Raw4<F>::t nr[J];          // (!XR: the front unit's y of the chunk's own elements, for its reduction)
        if constexpr (!XR) {
#pragma unroll
            for (int m = 0; m < J; ++m) nr[m] = sld4_raw<F>(nx.y, (long)(t0 + m * d < T ? off0 + (unsigned)m * rowstep : off0));
        }
        f32x4 dy2 = zero, dy1 = zero, xa2 = zero, xa1 = zero;      // windows: elements k - 2, k - 1
#pragma unroll
        for (int k = 0; k < J + 2; ++k) {
            const int tf = t0 + k * d, tb = t0 + (k - 2) * d;
            // dy of forward element k (zero past the utterance)
            f32x4 dy0;
            {
                const f32x4 xh = (dec4<F>(yr[k]) - mean) * istd, z = gm * xh + bt;
                const f32x4 gv = dec4<GF>(gr[k]), gs = sl * gv;
                f32x4 dz;
#pragma unroll
                for (int e = 0; e < 4; ++e) dz[e] = z[e] > 0.f ? gv[e] : gs[e];
                dy0 = gi * (dz - m1 - xh * m2);
                dy0 = tf < T ? dy0 : zero;
            }
            // the unit's input x of backward element k - 2 (zero outside the utterance), and the front unit's z / xhat there
            f32x4 xa0, nz = zero, nxh = zero;
            if constexpr (XR) {
                nxh = (dec4<F>(br[k]) - nmean) * nistd;
                nz = ngm * nxh + nbt;
#pragma unroll
                for (int e = 0; e < 4; ++e) xa0[e] = nz[e] > 0.f ? nz[e] : nsl * nz[e];
                if (nx.xround) xa0 = round_bf4(xa0, 1);
            } else {
                xa0 = dec4<F>(br[k]);
            }
            xa0 = (tb >= 0 && tb < T) ? xa0 : zero;
            if (k >= 2) {
                // output element m = k - 2 (frame tb): dy window (dy2, dy1, dy0) = elements m, m + 1, m + 2; x window
                // (xa2, xa1, xa0) = elements m - 2, m - 1, m
                vwv[0] += dy2 * xa2;
                vwv[1] += dy2 * xa1;
                vwv[2] += dy2 * xa0;
                vwv[3] += dy2;
                if (tb < T) {
                    f32x4 acc = zero;
                    acc = acc + wk[0] * dy0;
                    acc = acc + wk[1] * dy1;
                    acc = acc + wk[2] * dy2;
                    acc = round_bf4(acc, GF);
                    sst4<kNtSt>(dx, (long)(off0 + (unsigned)(k - 2) * rowstep), GF, acc);
                    if constexpr (!XR) {
                        nxh = (dec4<F>(nr[k - 2 < J ? k - 2 : 0]) - nmean) * nistd;
                        nz = ngm * nxh + nbt;
                    }
                    const f32x4 as = nsl * acc, az = acc * nz;
                    f32x4 dz2, ds2;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool pos = nz[e] > 0.f;
                        dz2[e] = pos ? acc[e] : as[e];
                        ds2[e] = pos ? 0.f : az[e];
                    }
                    vrv[0] += dz2;
                    vrv[1] += dz2 * nxh;
                    vrv[2] += ds2;
                }
            }
            dy2 = dy1; dy1 = dy0;
            xa2 = xa1; xa1 = xa0;
        }
    }
    float vw[4][4], vr[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        vw[0][e] = vwv[0][e]; vw[1][e] = vwv[1][e]; vw[2][e] = vwv[2][e]; vw[3][e] = vwv[3][e];
        vr[0][e] = vrv[0][e]; vr[1][e] = vrv[1][e]; vr[2][e] = vrv[2][e];
    }
    block_reduce_store<4, 4>(vw, 16, sh, wpartial + (long)blockIdx.x * 64);
    block_reduce_store<3, 4>(vr, 16, sh, rpartial + (long)blockIdx.x * 48, fa.kind != 0);
    if (fa.kind) fin_reduce(rpartial, 48, (int)blockIdx.x, gridDim.x, fa);
}

// ---------------------------------------------- depth_conv FORWARD with point_conv1's BatchNorm + PReLU applied while staging
// point_conv1 -> depth_conv could not use the normalise-on-load forms above: nine taps would each re-apply the BatchNorm +
// PReLU (measured: slower than the separate k_bn_act pass).  With an LDS tile the activation is formed ONCE per element
// while the tile is staged -- the expressions of k_bn_act (pre_apply): bit-identical values -- the nine taps read it from
// LDS, and the owned rows go out to the saved activation (and, exact chain, the centred copy of y) as the separate pass
// wrote them.  k_bn_act (read y, write a) + a conv that re-reads a through nine global taps become one pass: read y, write
// a, write the conv output.  Same accumulation order as k_dw16 / k_conv_mfma (bias first, taps kt-major): the conv outputs
// are bit-identical; the BatchNorm partial sums are taken in double as there.
constexpr int F33_TF = 12, F33_ROWS = F33_TF + 2;
// stages rows r = input frames t0 - 2 + r (zero outside [0, T)) of utterance b into img [F33_ROWS][35][16] (pads untouched)
template <int FIN, int NTH>
__device__ __forceinline__ void stage_pre_tile(float* img, const float* __restrict__ in, const BnPre& pre, const PreConst& pk, int b,
                                               int t0, int T, int tid, int q) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    // (every load of the tile is issued before the first is used: UN covers the tile in one trip)
    constexpr int ITEMS = F33_ROWS * 33 * 4, UN = (ITEMS + NTH - 1) / NTH;
    for (int it0 = tid; it0 < ITEMS; it0 += UN * NTH) {              // (NTH % 4 == 0: every item's quad is q)
        typename Raw4<FIN>::t yr[UN];
        long idx[UN];
        int rec[UN], rr[UN];
        bool ok[UN], live[UN];
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            const int it = it0 + j * NTH;
            live[j] = it < ITEMS;
            const int pos = (live[j] ? it : 0) >> 2, r = pos / 33, f = pos - r * 33, tx = t0 - 2 + r;
            ok[j] = tx >= 0 && tx < T;
            idx[j] = (((long)b * T + (ok[j] ? tx : 0)) * 33 + f) * 16 + 4 * q;
            yr[j] = sld4_raw<FIN, true>(in, idx[j]);
            rec[j] = (r * 35 + 1 + f) * 16 + 4 * q;
            rr[j] = r;
        }
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            const f32x4 yraw = dec4<FIN>(yr[j]);
            const f32x4 a = pre_apply(pk, yraw, pre.exact ? 0 : pre.bf);
            if (live[j]) {
                *reinterpret_cast<f32x4*>(img + rec[j]) = ok[j] ? a : zero;
                if (ok[j] && rr[j] >= 2) {                              // the tile's own frames: each element once
                    pre_store(pre, idx[j], a);
                    pre_store_y(pre, pk, idx[j], yraw, false, zero);
                }
            }
        }
    }
}
template <int FIN>
__global__ __launch_bounds__(NT) void k_dw33_fwd_pre(DwGeom g, const float* __restrict__ in, const float* __restrict__ w,
                                                    const float* __restrict__ bias, float* __restrict__ out,
                                                    double* __restrict__ stat_partial, const float* __restrict__ shift,
                                                    BnPre pre, int tiles_t, FinArgs fa) {
    __shared__ __attribute__((aligned(16))) float sA[F33_ROWS * 35 * 16];
    __shared__ __attribute__((aligned(16))) float sW[9 * 16];       // [tap][c]
    __shared__ double sStat[NT / 64][32];
    const int tid = threadIdx.x, q = tid & 3;
    for (int i = tid; i < 9 * 16; i += NT) {
        const int tap = i >> 4, c = i & 15;
        sW[i] = w[c * g.w_c + (tap / 3) * g.w_kt + (tap % 3) * g.w_kf];
    }
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < F33_ROWS * 2 * 4; i += NT) {
        const int qq = i & 3, side = (i >> 2) & 1, r = i >> 3;
        *reinterpret_cast<f32x4*>(sA + (r * 35 + side * 34) * 16 + 4 * qq) = zero;
    }
    const PreConst pk = pre_const(pre, q, 16);
    f32x4 b0 = zero;
    if (bias) b0 = *reinterpret_cast<const f32x4*>(bias + 4 * q);
    if (shift) b0 -= *reinterpret_cast<const f32x4*>(shift + 4 * q);
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    const int T = g.Tout;
    const long ntiles = (long)g.B * tiles_t;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int b = (int)(tile / tiles_t), t0 = (int)(tile - (long)b * tiles_t) * F33_TF;
        __syncthreads();
        stage_pre_tile<FIN, NT>(sA, in, pre, pk, b, t0, T, tid, q);
        __syncthreads();
        const int nrow = T - t0 < F33_TF ? T - t0 : F33_TF;
        for (int it = tid; it < nrow * 33 * 4; it += NT) {
            const int pos = it >> 2, r = pos / 33, f = pos - r * 33;
            const long p = ((long)b * T + t0 + r) * 33 + f;
            const float* aq = sA + (r * 35 + f) * 16 + 4 * q;       // tap (kt, kf): input frame t - 2 + kt, bin f - 1 + kf
            f32x4 acc = b0;
#pragma unroll
            for (int kt = 0; kt < 3; ++kt)
#pragma unroll
                for (int kf = 0; kf < 3; ++kf)
                    acc = acc + *reinterpret_cast<const f32x4*>(sW + (kt * 3 + kf) * 16 + 4 * q) *
                                    *reinterpret_cast<const f32x4*>(aq + (kt * 35 + kf) * 16);
            if (g.out_bf) {
                acc = round_bf4(acc, g.out_bf);
                sst4<kNtSt>(out, p * 16 + 4 * q, g.out_bf, acc);
            } else {
                sst4<kNtSt>(out, p * 16 + 4 * q, 0, acc);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) { const double a = (double)acc[e]; s1[e] += a; s2[e] = fma(a, a, s2[e]); }
        }
    }
    if (stat_partial) {   // per-workgroup BatchNorm partial sums; a thread's channel quad is tid & 3 (as k_dw16)
#pragma unroll
        for (int e = 0; e < 4; ++e) { s1[e] = wave_sum_xor(s1[e], 4, 32); s2[e] = wave_sum_xor(s2[e], 4, 32); }
        if ((tid & 63) < 4)
#pragma unroll
            for (int e = 0; e < 4; ++e) { sStat[tid >> 6][4 * q + e] = s1[e]; sStat[tid >> 6][16 + 4 * q + e] = s2[e]; }
        __syncthreads();
        if (tid < 32) {
            double t = 0.0;
            for (int w2 = 0; w2 < NT / 64; ++w2) t += sStat[w2][tid];
            st_part(stat_partial + (long)blockIdx.x * 32 + tid, t, fa);
        }
        if (fa.kind) fin_reduce(stat_partial, 32, blockIdx.x, gridDim.x, fa);
    }
}
// the decoder's dense transposed 3x3: y[to][fo] = b + sum W[kt][kf] a[to - kt][fo + 1 - kf], T + 2 output frames; per 16 output
// positions 36 MFMAs whose B operands are ds_read_b128 of the staged activation
template <int FIN>
__global__ __launch_bounds__(NT) void k_dense33_fwd_pre(ConvGeom g, const float* __restrict__ in, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ out,
                                                       double* __restrict__ stat_partial, const float* __restrict__ shift,
                                                       BnPre pre, int tiles_t, FinArgs fa) {
    __shared__ __attribute__((aligned(16))) float sA[F33_ROWS * 35 * 16];
    __shared__ __attribute__((aligned(16))) float sW[9 * 256];      // [tap][co][ci]
    __shared__ double sStat[NT / 64][32];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 15, q = lane >> 4, qs = tid & 3;
    for (int i = tid; i < 9 * 256; i += NT) {
        const int tap = i >> 8, co = (i >> 4) & 15, ci = i & 15;
        sW[i] = w[co * g.w_co + ci * g.w_ci + (tap / 3) * g.w_kt + (tap % 3) * g.w_kf];
    }
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < F33_ROWS * 2 * 4; i += NT) {
        const int qq = i & 3, side = (i >> 2) & 1, r = i >> 3;
        *reinterpret_cast<f32x4*>(sA + (r * 35 + side * 34) * 16 + 4 * qq) = zero;
    }
    const PreConst pk = pre_const(pre, qs, 16);
    f32x4 bv = zero;
    if (bias) bv = *reinterpret_cast<const f32x4*>(bias + 4 * q);
    if (shift) bv -= *reinterpret_cast<const f32x4*>(shift + 4 * q);
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    const int T = g.Tin, T2 = g.Tout;
    const long ntiles = (long)g.B * tiles_t;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int b = (int)(tile / tiles_t), t0 = (int)(tile - (long)b * tiles_t) * F33_TF;
        __syncthreads();
        stage_pre_tile<FIN, NT>(sA, in, pre, pk, b, t0, T, tid, qs);
        __syncthreads();
        const int own = (T2 - t0 < F33_TF ? T2 - t0 : F33_TF) * 33;
        for (int nt = wv; nt * 16 < own; nt += NT / 64) {
            const int pl = nt * 16 + n, pc = pl < own ? pl : 0, r = pc / 33, f = pc - r * 33;
            const long p = ((long)b * T2 + t0 + r) * 33 + f;
            const float* aq = sA + ((r + 2) * 35 + f + 2) * 16 + 4 * q;    // tap (kt, kf): a[to - kt][fo + 1 - kf]
            f32x4 acc = bv;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const f32x4 A = *reinterpret_cast<const f32x4*>(sW + tap * 256 + n * 16 + 4 * q);
                const f32x4 Bq = *reinterpret_cast<const f32x4*>(aq - ((tap / 3) * 35 + tap % 3) * 16);
#pragma unroll
                for (int s2i = 0; s2i < 4; ++s2i) acc = mfma4(A[s2i], Bq[s2i], acc);
            }
            if (pl < own) {
                if (g.out_bf) {
                    acc = round_bf4(acc, g.out_bf);
                    sst4<kNtSt>(out, p * 16 + 4 * q, g.out_bf, acc);
                } else {
                    sst4<kNtSt>(out, p * 16 + 4 * q, 0, acc);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) { const double a = (double)acc[e]; s1[e] += a; s2[e] = fma(a, a, s2[e]); }
            }
        }
    }
    if (stat_partial) {   // as k_conv_mfma: lanes of one channel quad differ in n (xor distances 8..1), then the waves through LDS
#pragma unroll
        for (int e = 0; e < 4; ++e) { s1[e] = wave_sum_xor(s1[e], 1, 8); s2[e] = wave_sum_xor(s2[e], 1, 8); }
        if (n == 0)
#pragma unroll
            for (int e = 0; e < 4; ++e) { sStat[wv][4 * q + e] = s1[e]; sStat[wv][16 + 4 * q + e] = s2[e]; }
        __syncthreads();
        if (tid < 32) {
            double t = 0.0;
            for (int w2 = 0; w2 < NT / 64; ++w2) t += sStat[w2][tid];
            st_part(stat_partial + (long)blockIdx.x * 32 + tid, t, fa);
        }
        if (fa.kind) fin_reduce(stat_partial, 32, blockIdx.x, gridDim.x, fa);
    }
}

// ------------------------------------------ fused backward of a depthwise 3x3 conv + BatchNorm + PReLU (encoder depth_conv)
// After the BatchNorm reduction the unit's three remaining passes -- dy (k_bn_bwd_apply: read da, y, write dy), the weight
// gradient (k_dw_wgrad_stream<3,3>: read dy, x at nine taps) and the data gradient (k_dw16<3,3> on the adjoint taps: read
// dy at nine taps, write dx) -- as ONE pass over LDS tiles: a workgroup takes D33_TF frames of one utterance (all 33
// bins, 16 channels), forms dy for those frames and the two after them (what its dx rows need; 2 / D33_TF recomputed)
// into one LDS image, copies x of those frames and the two before them (what its dW terms need) into a second one
// (35-column rows: zero pads instead of bin-edge tests), and after one barrier every thread (position, channel quad)
// reads its nine dy taps and nine x taps from LDS: dy never exists in memory and da, y, x are read once.  Same per-element
// expressions and the same order of additions as the separate kernels.  NEXT: the unit in front (point_conv1) takes this dx
// as its da -- its first backward pass rides along as in k_dwunit31_bwd.
constexpr int D33_TF = 12, D33_ROWS = D33_TF + 2;
// XR (with NEXT): x IS that unit's activation and is rebuilt from its y while the tile is staged (see NextRedArgs).
template <int FX, int FY, bool NEXT, bool XR = false, int GF = 0>   // storage formats of x (an activation), of y / the next unit's y (conv outputs), of da / dx
__global__ __launch_bounds__(NT) void k_dwunit33_bwd(DwGeom g, const float* __restrict__ x, const float* __restrict__ y,
                                                    const float* __restrict__ da, BnBwdArgs bn,
                                                    const float* __restrict__ w, float* __restrict__ dx,
                                                    double* __restrict__ wpartial, NextRedArgs nx,
                                                    double* __restrict__ rpartial, int tiles_t, FinArgs fa) {
    __shared__ __attribute__((aligned(16))) float sDy[D33_ROWS * 35 * 16];   // row r = frame t0 + r, column 1 + bin
    __shared__ __attribute__((aligned(16))) float sXi[D33_ROWS * 35 * 16];   // row r = frame t0 - 2 + r
    __shared__ double sh[NT];
    const int tid = threadIdx.x, q = tid & 3;
    const f32x4 mean = *reinterpret_cast<const f32x4*>(bn.stats + 4 * q), istd = *reinterpret_cast<const f32x4*>(bn.stats + 16 + 4 * q);
    const f32x4 gm = *reinterpret_cast<const f32x4*>(bn.gamma + 4 * q), bt = *reinterpret_cast<const f32x4*>(bn.beta + 4 * q);
    const f32x4 m1 = *reinterpret_cast<const f32x4*>(bn.red + 4 * q), m2 = *reinterpret_cast<const f32x4*>(bn.red + 16 + 4 * q);
    const float sl = bn.slope[0];
    f32x4 wk[9];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) wk[k][e] = w[(4 * q + e) * g.w_c + (k / 3) * g.w_kt + (k % 3) * g.w_kf];
    NextConst nk{};
    if constexpr (NEXT) nk = next_const(nx, 4 * q);
    float vw[10][4], vr[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int k = 0; k < 10; ++k) vw[k][e] = 0.f;
        vr[0][e] = vr[1][e] = vr[2][e] = 0.f;
    }
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < D33_ROWS * 2 * 4 * 2; i += NT) {          // pad columns 0 and 34 of both images, once
        const int qq = i & 3, side = (i >> 2) & 1, r = (i >> 3) % D33_ROWS, img = i / (8 * D33_ROWS);
        *reinterpret_cast<f32x4*>((img ? sXi : sDy) + (r * 35 + side * 34) * 16 + 4 * qq) = zero;
    }
    const int T = g.Tout, F = g.F;                                   // F == 33: the launcher checks
    const long ntiles = (long)g.B * tiles_t;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int b = (int)(tile / tiles_t), t0 = (int)(tile - (long)b * tiles_t) * D33_TF;
        const long rowb = (long)b * T;
        __syncthreads();                                             // the previous tile's readers are done
        // ---- stage 1: dy of frames t0 .. t0 + D33_ROWS - 1, x of frames t0 - 2 .. t0 + D33_ROWS - 3 (zero outside the tensor)
        for (int it = tid; it < D33_ROWS * 33 * 4; it += NT) {       // (NT % 4 == 0: the item's quad is the thread's)
            const int pos = it >> 2, r = pos / 33, f = pos - r * 33;
            const int td = t0 + r, tx = t0 - 2 + r;
            const bool okd = td < T, okx = tx >= 0 && tx < T;
            const long pd = (rowb + (okd ? td : 0)) * F + f, px = (rowb + (okx ? tx : 0)) * F + f;
            const typename Raw4<FY>::t yr = sld4_raw<FY, true>(y, pd * 16 + 4 * q);
            const typename Raw4<GF>::t grr = sld4_raw<GF, true>(da, pd * 16 + 4 * q);
            typename Raw4<FX>::t xr{};
            typename Raw4<FY>::t xyr{};
            static_assert(!XR || NEXT, "x is rebuilt from the NEXT unit's y");
            if constexpr (XR) xyr = sld4_raw<FY, true>(nx.y, px * 16 + 4 * q);
            else xr = sld4_raw<FX, true>(x, px * 16 + 4 * q);
            const f32x4 yv = dec4<FY>(yr);
            const f32x4 gr = dec4<GF>(grr);
            f32x4 dyv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xh = (yv[e] - mean[e]) * istd[e];
                const float z = gm[e] * xh + bt[e];
                const float dz = z > 0.f ? gr[e] : sl * gr[e];
                dyv[e] = gm[e] * istd[e] * (dz - m1[e] - xh * m2[e]);
            }
            *reinterpret_cast<f32x4*>(sDy + (r * 35 + 1 + f) * 16 + 4 * q) = okd ? dyv : zero;
            f32x4 xval;
            if constexpr (XR) xval = next_act(nk, dec4<FY>(xyr), nx.xround);
            else xval = dec4<FX>(xr);
            *reinterpret_cast<f32x4*>(sXi + (r * 35 + 1 + f) * 16 + 4 * q) = okx ? xval : zero;
        }
        __syncthreads();
        // ---- stage 2: the tile's own frames t0 .. t0 + D33_TF - 1
        const int nrow = T - t0 < D33_TF ? T - t0 : D33_TF;
        for (int it = tid; it < nrow * 33 * 4; it += NT) {
            const int pos = it >> 2, r = pos / 33, f = pos - r * 33;
            const long p = (rowb + t0 + r) * F + f;
            typename Raw4<FY>::t ynr{};
            if constexpr (NEXT) ynr = sld4_raw<FY, true>(nx.y, p * 16 + 4 * q);
            // dx(t, f) = sum w[kt][kf] dy(t + 2 - kt, f + 1 - kf): the adjoint taps in the order of k_dw16
            const float* dq = sDy + (r * 35 + 1 + f) * 16 + 4 * q;
            f32x4 acc = zero;
#pragma unroll
            for (int kt = 0; kt < 3; ++kt)
#pragma unroll
                for (int kf = 0; kf < 3; ++kf)
                    acc = acc + wk[kt * 3 + kf] * *reinterpret_cast<const f32x4*>(dq + ((2 - kt) * 35 + 1 - kf) * 16);
            acc = round_bf4(acc, GF);
            sst4<kNtSt>(dx, p * 16 + 4 * q, GF, acc);
            if constexpr (NEXT) next_accum(nk, dec4<FY>(ynr), acc, vr);
            // dW[kt][kf] += dy(t, f) x(t - 2 + kt, f - 1 + kf); db += dy(t, f)
            const f32x4 d = *reinterpret_cast<const f32x4*>(dq);
            const float* xq = sXi + (r * 35 + 1 + f) * 16 + 4 * q;
#pragma unroll
            for (int kt = 0; kt < 3; ++kt)
#pragma unroll
                for (int kf = 0; kf < 3; ++kf) {
                    const f32x4 xv = *reinterpret_cast<const f32x4*>(xq + (kt * 35 + kf - 1) * 16);
#pragma unroll
                    for (int e = 0; e < 4; ++e) vw[kt * 3 + kf][e] = fmaf(d[e], xv[e], vw[kt * 3 + kf][e]);
                }
#pragma unroll
            for (int e = 0; e < 4; ++e) vw[9][e] += d[e];
        }
    }
    block_reduce_store<10, 4>(vw, 16, sh, wpartial + (long)blockIdx.x * 160);
    if constexpr (NEXT) {
        block_reduce_store<3, 4>(vr, 16, sh, rpartial + (long)blockIdx.x * 48, fa.kind != 0);
        if (fa.kind) fin_reduce(rpartial, 48, blockIdx.x, gridDim.x, fa);
    }
}

// ------------------------------------------ fused backward of the dense transposed 3x3 conv + BatchNorm + PReLU (decoder depth_conv)
// The same LDS tiling for the decoder's depth_conv (ConvTranspose2d(16,16,(3,3)): y[to][fo] = sum W[kt][kf] x[to - kt][fo + 1 - kf],
// T + 2 output frames).  After the BatchNorm reduction: k_bn_bwd_apply (read da, y, write dy) + k_conv_wgrad_lds<3,3> (read dy, x at
// nine taps) + the adjoint k_conv_mfma<3,3> (read dy at nine taps, write dx) were three latency-bound passes over global
// memory (2.3-2.5 TB/s).  Here a workgroup forms dy of D9_TF + 2 frames into one LDS image, copies x of the same span (two
// frames earlier) into a second, and both matrix products take their operands from LDS:
//   dx[ti][fi] = sum_taps W[tap]^T dy[ti + kt][fi - 1 + kf]       36 MFMAs per 16 positions, B operand = one ds_read_b128 per tap
//   dW[tap]   += dy[to][fo] (x) x[to - kt][fo + 1 - kf]            36 MFMAs per 16 positions, positions as the K index (lane (c, k)
//                                                                  reads channel c of position 4u + k of either image)
// in the accumulation order of the separate kernels (tap-major chains).  NEXT: point_conv1's reduction rides on dx.
// 596 us per launch against 860 for the three passes.  Timed apart (same launch with one stage compiled out): the fill alone
// 186 us, the matrix stage alone 444 us (its MFMAs alone would be 252): the stages barely overlap and the matrix stage runs
// at 57 % of the pipe (fp32 MFMA does not co-issue with the index / reduction VALU work; 25 position tiles on 4 waves).
// Tried on top, none faster: six waves per workgroup, the next tile's fill prefetched into registers (the riding
// reduction's own load then waits for the whole prefetch: vmcnt retires in order), producer / matrix wave specialisation
// with double-buffered images (one workgroup per CU: -0.54 ms per step against -0.78), staggering the two workgroups of a CU.
constexpr int D9_TF = 12, D9_ROWS = D9_TF + 2, D9_IMG = D9_ROWS * 35 * 16;
constexpr int D9_LDS_FLOATS = 2 * D9_IMG + 9 * 256;
static_assert(D9_LDS_FLOATS * 4 * 2 <= 160 * 1024, "two workgroups per CU");
static_assert((NT / 64) * (9 * 256 + 64) <= 2 * D9_IMG, "the accumulator tiles reuse the images");
template <int FX, int FY, bool NEXT, bool XR = false, int GF = 0>      // XR, GF: see k_dwunit33_bwd
// (two workgroups per CU by LDS: keep the register file at two waves per SIMD -- left alone the compiler gave the fp32
// recomputing form 234 + 40 registers, one wave per SIMD, and the kernel took 770 us instead of 580)
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2))) void k_dense33_bwd(ConvGeom g, const float* __restrict__ x, const float* __restrict__ y,
                                                   const float* __restrict__ da, BnBwdArgs bn,
                                                   const float* __restrict__ w, float* __restrict__ dx,
                                                   float* __restrict__ wpartial, NextRedArgs nx,
                                                   double* __restrict__ rpartial, int tiles_t, FinArgs fa) {
    extern __shared__ __attribute__((aligned(16))) float smem_d9[];
    float* sDy = smem_d9;                  // row r = dy frame t0 + r, column 1 + bin (pads 0, 34)
    float* sXi = sDy + D9_IMG;             // row r = x frame t0 - 2 + r
    float* sWa = sXi + D9_IMG;             // [tap][ci][co]: the A fragments of the data gradient
    __shared__ double sRed[NEXT ? NT / 64 : 1][48];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 15, q = lane >> 4, qs = tid & 3;
    for (int i = tid; i < 9 * 256; i += NT) {
        const int tap = i >> 8, ci = (i >> 4) & 15, co = i & 15;
        sWa[i] = w[co * g.w_co + ci * g.w_ci + (tap / 3) * g.w_kt + (tap % 3) * g.w_kf];
    }
    const f32x4 mean = *reinterpret_cast<const f32x4*>(bn.stats + 4 * qs), istd = *reinterpret_cast<const f32x4*>(bn.stats + 16 + 4 * qs);
    const f32x4 gm = *reinterpret_cast<const f32x4*>(bn.gamma + 4 * qs), bt = *reinterpret_cast<const f32x4*>(bn.beta + 4 * qs);
    const f32x4 m1 = *reinterpret_cast<const f32x4*>(bn.red + 4 * qs), m2 = *reinterpret_cast<const f32x4*>(bn.red + 16 + 4 * qs);
    const float sl = bn.slope[0];
    NextConst nk{}, nks{};
    if constexpr (NEXT) nk = next_const(nx, 4 * q);
    if constexpr (XR) nks = next_const(nx, 4 * qs);        // (the staging quad)
    static_assert(!XR || NEXT, "x is rebuilt from the NEXT unit's y");
    float vr[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) vr[0][e] = vr[1][e] = vr[2][e] = 0.f;
    f32x4 accW[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) accW[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < D9_ROWS * 2 * 4 * 2; i += NT) {          // pad columns 0 and 34 of both images, once
        const int qq = i & 3, side = (i >> 2) & 1, r = (i >> 3) % D9_ROWS, img = i / (8 * D9_ROWS);
        *reinterpret_cast<f32x4*>((img ? sXi : sDy) + (r * 35 + side * 34) * 16 + 4 * qq) = zero;
    }
    const int T = g.Tin, T2 = g.Tout;                              // x frames, dy frames (T + 2); 33 bins: the launcher checks
    const long ntiles = (long)g.B * tiles_t;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int b = (int)(tile / tiles_t), t0 = (int)(tile - (long)b * tiles_t) * D9_TF;
        __syncthreads();                                             // the previous tile's readers are done
        // ---- stage 1: dy of frames t0 .. t0 + D9_ROWS - 1, x of frames t0 - 2 .. t0 + D9_ROWS - 3 (zero outside the tensors)
        {   // (every load of the tile first: one item at a time the fill was a chain of exposed round trips)
            constexpr int ITEMS = D9_ROWS * 33 * 4, NI = (ITEMS + NT - 1) / NT;      // (NT % 4 == 0: every item's quad is qs)
            typename Raw4<FY>::t yr[NI];
            typename Raw4<GF>::t gr[NI];
            typename Raw4<FX>::t xr[NI];
            typename Raw4<FY>::t xyr[NI];
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const int it = tid + j * NT, pos = (it < ITEMS ? it : 0) >> 2, r = pos / 33, f = pos - r * 33;
                const int td = t0 + r, tx = t0 - 2 + r;
                const long pd = ((long)b * T2 + (td < T2 ? td : 0)) * 33 + f, px = ((long)b * T + ((tx >= 0 && tx < T) ? tx : 0)) * 33 + f;
                yr[j] = sld4_raw<FY, true>(y, pd * 16 + 4 * qs);
                gr[j] = sld4_raw<GF, true>(da, pd * 16 + 4 * qs);
                if constexpr (XR) xyr[j] = sld4_raw<FY, true>(nx.y, px * 16 + 4 * qs);
                else xr[j] = sld4_raw<FX, true>(x, px * 16 + 4 * qs);
            }
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const int it = tid + j * NT, pos = (it < ITEMS ? it : 0) >> 2, r = pos / 33, f = pos - r * 33;
                const int td = t0 + r, tx = t0 - 2 + r;
                const f32x4 yv = dec4<FY>(yr[j]);
                const f32x4 gj = dec4<GF>(gr[j]);
                f32x4 dyv;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float xh = (yv[e] - mean[e]) * istd[e];
                    const float z = gm[e] * xh + bt[e];
                    const float dz = z > 0.f ? gj[e] : sl * gj[e];
                    dyv[e] = gm[e] * istd[e] * (dz - m1[e] - xh * m2[e]);
                }
                f32x4 xval;
                if constexpr (XR) xval = next_act(nks, dec4<FY>(xyr[j]), nx.xround);
                else xval = dec4<FX>(xr[j]);
                if (it < ITEMS) {
                    *reinterpret_cast<f32x4*>(sDy + (r * 35 + 1 + f) * 16 + 4 * qs) = td < T2 ? dyv : zero;
                    *reinterpret_cast<f32x4*>(sXi + (r * 35 + 1 + f) * 16 + 4 * qs) = (tx >= 0 && tx < T) ? xval : zero;
                }
            }
        }
        __syncthreads();
        // ---- stage 2: 16-position tiles of the D9_TF x 33 owned positions, one wave each
        const int own_x = (T - t0 < D9_TF ? (T - t0 > 0 ? T - t0 : 0) : D9_TF) * 33;      // positions whose dx this tile writes
        const int own_d = (T2 - t0 < D9_TF ? T2 - t0 : D9_TF) * 33;                        // dy positions whose dW terms it adds
        for (int nt = wv; nt * 16 < own_d; nt += NT / 64) {
            if (nt * 16 < own_x) {
                // data gradient of position pl (lane (n, q): input channels 4q .. 4q + 3)
                const int pl = nt * 16 + n, pc = pl < own_x ? pl : 0, r = pc / 33, f = pc - r * 33;
                const long gp = ((long)b * T + t0 + r) * 33 + f;
                typename Raw4<FY>::t ynr{};
                if constexpr (NEXT) ynr = sld4_raw<FY, true>(nx.y, gp * 16 + 4 * q);
                const float* dq = sDy + (r * 35 + f) * 16 + 4 * q;
                f32x4 acc = zero;
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const f32x4 A = *reinterpret_cast<const f32x4*>(sWa + tap * 256 + n * 16 + 4 * q);
                    const f32x4 Bv = *reinterpret_cast<const f32x4*>(dq + ((tap / 3) * 35 + tap % 3) * 16);   // dy[ti + kt][fi - 1 + kf]
#pragma unroll
                    for (int s2 = 0; s2 < 4; ++s2) acc = mfma4(A[s2], Bv[s2], acc);
                }
                if (pl < own_x) {
                    acc = round_bf4(acc, GF);
                    sst4<kNtSt>(dx, gp * 16 + 4 * q, GF, acc);
                    if constexpr (NEXT) next_accum(nk, dec4<FY>(ynr), acc, vr);
                }
            }
            // weight gradient: lane (c = n, k = q) takes channel c of positions 4u + k
            // (all forty operand reads of the sixteen positions first, then the 36 MFMAs: read-then-use per MFMA left the
            // matrix pipe waiting for an LDS round trip every one or two instructions)
            float av[4], bv[4][9];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int pu = nt * 16 + 4 * u + q, pc = pu < own_d ? pu : 0, r = pc / 33, f = pc - r * 33;
                const float a = sDy[(r * 35 + 1 + f) * 16 + n];
                av[u] = pu < own_d ? a : 0.f;
                const float* xq = sXi + ((r + 2) * 35 + f + 2) * 16 + n;       // x[to - kt][fo + 1 - kf] at row + 2 - kt, column + 2 - kf
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) bv[u][tap] = xq[-((tap / 3) * 35 + tap % 3) * 16];
            }
            __builtin_amdgcn_sched_barrier(0);        // (the scheduler interleaves them again otherwise)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                bsum += av[u];
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) accW[tap] = mfma4(av[u], bv[u][tap], accW[tap]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    __syncthreads();                                                 // the images are dead: the accumulators go there
    float* my = smem_d9 + wv * (9 * 256 + 64);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int r = 0; r < 4; ++r) my[tap * 256 + (4 * q + r) * 16 + n] = accW[tap][r];
    my[9 * 256 + lane] = bsum;
    __syncthreads();
    float* pp = wpartial + (long)blockIdx.x * (9 * 256 + 16);
    for (int i = tid; i < 9 * 256; i += NT) {
        float t = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < NT / 64; ++w2) t += smem_d9[w2 * (9 * 256 + 64) + i];
        pp[i] = t;
    }
    if (tid < 16) {
        float t = 0.f;
        for (int w2 = 0; w2 < NT / 64; ++w2)
            for (int kk = 0; kk < 4; ++kk) t += smem_d9[w2 * (9 * 256 + 64) + 9 * 256 + kk * 16 + tid];
        pp[9 * 256 + tid] = t;
    }
    if constexpr (NEXT) {
#pragma unroll
        for (int k3 = 0; k3 < 3; ++k3)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double t = wave_sum_xor((double)vr[k3][e], 1, 8);
                if (n == 0) sRed[wv][k3 * 16 + 4 * q + e] = t;
            }
        __syncthreads();
        if (tid < 48) {
            double t = 0.0;
            for (int w2 = 0; w2 < NT / 64; ++w2) t += sRed[w2][tid];
            st_part(rpartial + (long)blockIdx.x * 48 + tid, t, fa);
        }
        if (fa.kind) fin_reduce(rpartial, 48, blockIdx.x, gridDim.x, fa);
    }
}

// ------------------------------------------ fused backward of the two 16 -> 16 (1,5) stride-2 units (en_convs.1, de_convs.3)
// en_convs.1 is Conv2d(16,16,(1,5),stride (1,2),padding (0,2)): y_n[fn] = sum_kf W[kf] x_w[2 fn - 2 + kf] (65 -> 33 bins);
// de_convs.3 is the ConvTranspose2d of the same shape: y_w[fw] = sum over (fn, kf) with fw = 2 fn - 2 + kf of W[kf] x_n[fn]
// (33 -> 65 bins).  Both couple a NARROW tensor (33 bins) with a WIDE one (65 bins) through the same index relation
// fw = 2 fn - 2 + kf, with dy on the narrow side for en_convs.1 and on the wide side for de_convs.3 (DYW).  Their backward
// was k_bn_bwd_apply (dy written) + k_conv_wgrad_lds<1,5> + the adjoint k_conv_mfma<1,5>: here a workgroup takes C15_TF
// frames of one utterance (no halo: the taps run along frequency only), forms dy from da, y into the LDS image of its side,
// copies x into the other image (rows padded with zero columns for the out-of-range taps), and both matrix products read
// LDS:   dW[kf] += dy (x) x over the 33 narrow positions of a frame       (positions as the MFMA K index)
//        dx     = sum_kf W[kf]^T dy[...]                                   (on the x side; en_convs.1: the wide side, where a
//                                                                         position meets taps of one parity only -- the other
//                                                                         taps enter as zero operands)
// dx may ACCUMULATE (en_convs.1: on top of the skip gradient of en_outs[0]) and carry the NEXT unit's riding reduction.
constexpr int C15_TF = 8, C15_NW = 33 + 2, C15_WW = 65 + 4;        // narrow rows: pads -1, 33; wide rows: pads -2, -1, 65, 66
constexpr int C15_NIMG = C15_TF * C15_NW * 16, C15_WIMG = C15_TF * C15_WW * 16;
template <bool DYW, int FX, int FY, int NEXT, int GF = 0>      // NEXT: 0 none, 1 + storage format of that unit's y; GF: see k_unit1x1_bwd
__global__ __launch_bounds__(NT) void k_conv15_bwd(ConvGeom g, const float* __restrict__ x, const float* __restrict__ y,
                                                  const float* __restrict__ da, BnBwdArgs bn,
                                                  const float* __restrict__ w, float* __restrict__ dx, int dx_acc,
                                                  float* __restrict__ wpartial, NextRedArgs nx,
                                                  double* __restrict__ rpartial, int tiles_t, FinArgs fa) {
    __shared__ __attribute__((aligned(16))) float sN[C15_NIMG];      // narrow side: column 1 + fn
    __shared__ __attribute__((aligned(16))) float sWd[C15_WIMG];     // wide side: column 2 + fw
    __shared__ __attribute__((aligned(16))) float sWa[5 * 256];      // [kf][ci][co]: A fragments of the data gradient
    __shared__ double sRed[NEXT ? NT / 64 : 1][48];
    __shared__ float sB[NT / 64][16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 15, q = lane >> 4, qs = tid & 3;
    for (int i = tid; i < 5 * 256; i += NT) {
        const int kf = i >> 8, ci = (i >> 4) & 15, co = i & 15;
        sWa[i] = w[co * g.w_co + ci * g.w_ci + kf * g.w_kf];
    }
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < C15_TF * 2 * 4; i += NT) {                 // narrow pads
        const int qq = i & 3, side = (i >> 2) & 1, r = i >> 3;
        *reinterpret_cast<f32x4*>(sN + (r * C15_NW + side * 34) * 16 + 4 * qq) = zero;
    }
    for (int i = tid; i < C15_TF * 4 * 4; i += NT) {                 // wide pads: columns 0, 1, 67, 68
        const int qq = i & 3, c4 = (i >> 2) & 3, r = i >> 4;
        *reinterpret_cast<f32x4*>(sWd + (r * C15_WW + (c4 < 2 ? c4 : 65 + c4)) * 16 + 4 * qq) = zero;
    }
    const f32x4 mean = *reinterpret_cast<const f32x4*>(bn.stats + 4 * qs), istd = *reinterpret_cast<const f32x4*>(bn.stats + 16 + 4 * qs);
    const f32x4 gm = *reinterpret_cast<const f32x4*>(bn.gamma + 4 * qs), bt = *reinterpret_cast<const f32x4*>(bn.beta + 4 * qs);
    const f32x4 m1 = *reinterpret_cast<const f32x4*>(bn.red + 4 * qs), m2 = *reinterpret_cast<const f32x4*>(bn.red + 16 + 4 * qs);
    const float sl = bn.slope[0];
    NextConst nk{};
    if constexpr (NEXT != 0) nk = next_const(nx, 4 * q);
    float vr[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) vr[0][e] = vr[1][e] = vr[2][e] = 0.f;
    f32x4 accW[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) accW[i] = zero;
    f32x4 bq = zero;                                                 // bias gradient of the staging quad
    float* sDyI = DYW ? sWd : sN;                                    // dy lives on the wide side for de_convs.3
    float* sXI = DYW ? sN : sWd;
    constexpr int FD = DYW ? 65 : 33, FXB = DYW ? 33 : 65;           // bins of dy / of x (and dx)
    constexpr int CD = DYW ? C15_WW : C15_NW, CX = DYW ? C15_NW : C15_WW, OD = DYW ? 2 : 1, OX = DYW ? 1 : 2;
    const int T = g.Tout;                                            // (Tin == Tout)
    const long ntiles = (long)g.B * tiles_t;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int b = (int)(tile / tiles_t), t0 = (int)(tile - (long)b * tiles_t) * C15_TF;
        const int nrow = T - t0 < C15_TF ? T - t0 : C15_TF;
        __syncthreads();
        // ---- stage 1: dy (from da, y) and x of the tile's frames; rows past the utterance's end are zero.  EVERY load of the
        //      tile is issued before the first is used (two items per trip were six exposed round trips per tile)
        {
            constexpr int ND = (C15_TF * FD * 4 + NT - 1) / NT, NX = (C15_TF * FXB * 4 + NT - 1) / NT;
            typename Raw4<FY>::t yr[ND];
            typename Raw4<GF>::t gr[ND];
            typename Raw4<FX>::t xr[NX];
#pragma unroll
            for (int j = 0; j < ND; ++j) {
                const int it = tid + j * NT, pos = (it < C15_TF * FD * 4 ? it : 0) >> 2, r = pos / FD, f = pos - r * FD;
                const long p = ((long)b * T + t0 + (r < nrow ? r : 0)) * FD + f;
                yr[j] = sld4_raw<FY, true>(y, p * 16 + 4 * qs);
                gr[j] = sld4_raw<GF, true>(da, p * 16 + 4 * qs);
            }
#pragma unroll
            for (int j = 0; j < NX; ++j) {
                const int it = tid + j * NT, pos = (it < C15_TF * FXB * 4 ? it : 0) >> 2, r = pos / FXB, f = pos - r * FXB;
                const long p = ((long)b * T + t0 + (r < nrow ? r : 0)) * FXB + f;
                xr[j] = sld4_raw<FX, true>(x, p * 16 + 4 * qs);
            }
#pragma unroll
            for (int j = 0; j < ND; ++j) {
                const int it = tid + j * NT, pos = (it < C15_TF * FD * 4 ? it : 0) >> 2, r = pos / FD, f = pos - r * FD;
                const f32x4 yv = dec4<FY>(yr[j]);
                const f32x4 gj = dec4<GF>(gr[j]);
                f32x4 dyv;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float xh = (yv[e] - mean[e]) * istd[e];
                    const float z = gm[e] * xh + bt[e];
                    const float dz = z > 0.f ? gj[e] : sl * gj[e];
                    dyv[e] = gm[e] * istd[e] * (dz - m1[e] - xh * m2[e]);
                }
                if (it < C15_TF * FD * 4) {
                    *reinterpret_cast<f32x4*>(sDyI + (r * CD + OD + f) * 16 + 4 * qs) = r < nrow ? dyv : zero;
                    if (r < nrow) bq = bq + dyv;
                }
            }
#pragma unroll
            for (int j = 0; j < NX; ++j) {
                const int it = tid + j * NT, pos = (it < C15_TF * FXB * 4 ? it : 0) >> 2, r = pos / FXB, f = pos - r * FXB;
                if (it < C15_TF * FXB * 4)
                    *reinterpret_cast<f32x4*>(sXI + (r * CX + OX + f) * 16 + 4 * qs) = r < nrow ? dec4<FX>(xr[j]) : zero;
            }
        }
        __syncthreads();
        // ---- stage 2a: weight gradient over the narrow positions (lane (c = n, k = q): channel c of positions 4u + k)
        const int ownn = nrow * 33;
        for (int nt = wv; nt * 16 < ownn; nt += NT / 64) {
            float av[4], bv[4][5];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int pu = nt * 16 + 4 * u + q, pc = pu < ownn ? pu : 0, r = pc / 33, fn = pc - r * 33;
                const float nar = sN[(r * C15_NW + 1 + fn) * 16 + n];
                av[u] = pu < ownn ? nar : 0.f;
                const float* wq = sWd + (r * C15_WW + 2 * fn) * 16 + n;            // wide bin 2 fn - 2 + kf at column 2 fn + kf
#pragma unroll
                for (int kf = 0; kf < 5; ++kf) bv[u][kf] = wq[kf * 16];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int kf = 0; kf < 5; ++kf) {
                    // D[co][ci]: the A operand carries dy, the B operand x
                    if constexpr (DYW) accW[kf] = mfma4(bv[u][kf], av[u], accW[kf]);
                    else accW[kf] = mfma4(av[u], bv[u][kf], accW[kf]);
                }
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- stage 2b: data gradient over the positions of x (lane (n, q): input channels 4q .. 4q + 3)
        const int ownx = nrow * FXB;
        for (int nt = wv; nt * 16 < ownx; nt += NT / 64) {
            const int pl = nt * 16 + n, pc = pl < ownx ? pl : 0, r = pc / FXB, f = pc - r * FXB;
            const long gp = ((long)b * T + t0 + r) * FXB + f;
            typename Raw4<(NEXT ? NEXT - 1 : 0)>::t ynr{};
            if constexpr (NEXT != 0) ynr = sld4_raw<(NEXT ? NEXT - 1 : 0), true>(nx.y, gp * 16 + 4 * q);
            f32x4 old = zero;
            if (dx_acc) old = sld4(dx, gp * 16 + 4 * q, GF);
            f32x4 acc = zero;
#pragma unroll
            for (int kf = 0; kf < 5; ++kf) {
                const f32x4 A = *reinterpret_cast<const f32x4*>(sWa + kf * 256 + n * 16 + 4 * q);
                f32x4 Bv;
                if constexpr (DYW) {                     // x narrow, dy wide: dx[fn] = sum_kf W[kf]^T dy[2 fn - 2 + kf]
                    Bv = *reinterpret_cast<const f32x4*>(sWd + (r * C15_WW + 2 * f + kf) * 16 + 4 * q);
                } else {                                  // x wide, dy narrow: fn = (fw + 2 - kf) / 2 for the taps of fw's parity
                    const int num = f + 2 - kf;
                    const f32x4 v = *reinterpret_cast<const f32x4*>(sN + (r * C15_NW + 1 + (num >> 1)) * 16 + 4 * q);
                    Bv = (num & 1) ? zero : v;
                }
#pragma unroll
                for (int s2 = 0; s2 < 4; ++s2) acc = mfma4(A[s2], Bv[s2], acc);
            }
            if (pl < ownx) {
                acc = round_bf4(acc + old, GF);
                sst4<kNtSt>(dx, gp * 16 + 4 * q, GF, acc);
                if constexpr (NEXT != 0) next_accum(nk, dec4<(NEXT ? NEXT - 1 : 0)>(ynr), acc, vr);
            }
        }
    }
    __syncthreads();                                                 // the images are dead: the accumulators go there
    static_assert((NT / 64) * (5 * 256) <= C15_WIMG, "accumulator tiles fit in the wide image");
    float* my = sWd + wv * (5 * 256);
#pragma unroll
    for (int kf = 0; kf < 5; ++kf)
#pragma unroll
        for (int r = 0; r < 4; ++r) my[kf * 256 + (4 * q + r) * 16 + n] = accW[kf][r];
    // bias gradient: the staging quads' sums of dy (thread quad qs; lanes with equal qs differ in the other lane bits)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float t = bq[e];
        t += __shfl_xor(t, 4, 64); t += __shfl_xor(t, 8, 64); t += __shfl_xor(t, 16, 64); t += __shfl_xor(t, 32, 64);
        if (lane < 4) sB[wv][4 * lane + e] = t;
    }
    __syncthreads();
    float* pp = wpartial + (long)blockIdx.x * (5 * 256 + 16);
    for (int i = tid; i < 5 * 256; i += NT) {
        float t = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < NT / 64; ++w2) t += sWd[w2 * (5 * 256) + i];
        pp[i] = t;
    }
    if (tid < 16) {
        float t = 0.f;
        for (int w2 = 0; w2 < NT / 64; ++w2) t += sB[w2][tid];
        pp[5 * 256 + tid] = t;
    }
    if constexpr (NEXT != 0) {
#pragma unroll
        for (int k3 = 0; k3 < 3; ++k3)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double t = wave_sum_xor((double)vr[k3][e], 1, 8);
                if (n == 0) sRed[wv][k3 * 16 + 4 * q + e] = t;
            }
        __syncthreads();
        if (tid < 48) {
            double t = 0.0;
            for (int w2 = 0; w2 < NT / 64; ++w2) t += sRed[w2][tid];
            st_part(rpartial + (long)blockIdx.x * 48 + tid, t, fa);
        }
        if (fa.kind) fin_reduce(rpartial, 48, blockIdx.x, gridDim.x, fa);
    }
}

// --------------------------------------------------------------------------- features, mask
// GTCRNMicro.forward prologue + ERB.bm (models/gtcrn_micro.py:510-516, :63-67): one thread per (b,t,j)
// first / one-past-last non-zero entry of each of the `rows` rows (stride rs, element stride es) of a filterbank
__device__ __forceinline__ void nz_ranges(const float* w, int rows, int cols, int rs, int es, int* lo, int* hi) {
    for (int r = threadIdx.x; r < rows; r += blockDim.x) {
        int a = cols, b = 0;
        for (int i = 0; i < cols; ++i)
            if (w[(long)r * rs + (long)i * es] != 0.f) { if (i < a) a = i; b = i + 1; }
        lo[r] = a < b ? a : 0;
        hi[r] = b;
    }
    __syncthreads();
}

__global__ __launch_bounds__(NT) void k_feat(const float* __restrict__ spec, long sb, long sf, long st, int B, int T,
                                            const float* __restrict__ erb_w, float* __restrict__ eb, int bf,
                                            float* __restrict__ eb2, int eb2_bf) {
    __shared__ int lo[64], hi[64];
    nz_ranges(erb_w, 64, 192, 192, 1, lo, hi);
    const long total = (long)B * T * 129;
    for (long p = (long)blockIdx.x * NT + threadIdx.x; p < total; p += (long)gridDim.x * NT) {
        const int j = (int)(p % 129);
        const long bt = p / 129;
        const int t = (int)(bt % T), b = (int)(bt / T);
        const float* x = spec + (long)b * sb + (long)t * st;
        float m = 0.f, re = 0.f, im = 0.f;
        if (j < 65) {
            re = x[(long)j * sf]; im = x[(long)j * sf + 1];
            m = sqrtf(re * re + im * im + 1e-12f);
        } else {
            // (a band's bins requested together, then the multiply-adds in ascending-bin order: see k_feat_t; 373 -> 289 us
            // on frame-major spectrograms)
            constexpr int BW = 12;
            const float* w = erb_w + (long)(j - 65) * 192;
            const int l0 = lo[j - 65], h0 = hi[j - 65];
            float xr[BW], xq[BW], wv[BW];
#pragma unroll
            for (int u = 0; u < BW; ++u) {
                const int i = l0 + u < 192 ? l0 + u : 191;
                xr[u] = x[(long)(65 + i) * sf]; xq[u] = x[(long)(65 + i) * sf + 1];
                wv[u] = l0 + u < h0 ? w[i] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < BW; ++u) {
                m = fmaf(wv[u], sqrtf(xr[u] * xr[u] + xq[u] * xq[u] + 1e-12f), m);
                re = fmaf(wv[u], xr[u], re);
                im = fmaf(wv[u], xq[u], im);
            }
            for (int i = l0 + BW; i < h0; ++i) {
                const float wi = w[i];
                const float r = x[(long)(65 + i) * sf], q = x[(long)(65 + i) * sf + 1];
                m = fmaf(wi, sqrtf(r * r + q * q + 1e-12f), m);
                re = fmaf(wi, r, re);
                im = fmaf(wi, q, im);
            }
        }
        sst1(eb, p * 3, bf, m); sst1(eb, p * 3 + 1, bf, re); sst1(eb, p * 3 + 2, bf, im);
        if (eb2) { sst1(eb2, p * 3, eb2_bf, m); sst1(eb2, p * 3 + 1, eb2_bf, re); sst1(eb2, p * 3 + 2, eb2_bf, im); }
    }
}

// ERB.bs (:69-73) + Mask (:472-482) + output permute (:529-530): one thread per (b,t,f)
__global__ __launch_bounds__(NT) void k_bs_mask(const float* __restrict__ m, const float* __restrict__ spec, long sb,
                                               long sf, long st, int B, int T, const float* __restrict__ ierb_w,
                                               float* __restrict__ out, long ob, long of, long ot, int bf) {
    __shared__ int lo[192], hi[192];
    nz_ranges(ierb_w, 192, 64, 64, 1, lo, hi);
    const long total = (long)B * T * 257;
    for (long p = (long)blockIdx.x * NT + threadIdx.x; p < total; p += (long)gridDim.x * NT) {
        const int f = (int)(p % 257);
        const long bt = p / 257;
        const int t = (int)(bt % T), b = (int)(bt / T);
        const long mm = bt * 129 * 2;
        float m0 = 0.f, m1 = 0.f;
        if (f < 65) {
            m0 = sld1(m, mm + f * 2, bf); m1 = sld1(m, mm + f * 2 + 1, bf);
        } else {
            const float* w = ierb_w + (long)(f - 65) * 64;
            for (int j = lo[f - 65]; j < hi[f - 65]; ++j) {
                const float wj = w[j];
                if (wj != 0.f) {
                    m0 = fmaf(wj, sld1(m, mm + (65 + j) * 2, bf), m0);
                    m1 = fmaf(wj, sld1(m, mm + (65 + j) * 2 + 1, bf), m1);
                }
            }
        }
        const float* x = spec + (long)b * sb + (long)t * st + (long)f * sf;
        float* o = out + (long)b * ob + (long)t * ot + (long)f * of;
        o[0] = x[0] * m0 - x[1] * m1;
        o[1] = x[1] * m0 + x[0] * m1;
    }
}

__global__ __launch_bounds__(NT) void k_bs_mask_bwd(const float* __restrict__ dout, long ob, long of, long ot,
                                                   const float* __restrict__ spec, long sb, long sf, long st, int B,
                                                   int T, const float* __restrict__ ierb_w, float* __restrict__ dm) {
    __shared__ int lo[64], hi[64];
    nz_ranges(ierb_w, 64, 192, 1, 64, lo, hi);        // columns of the (192, 64) matrix
    const long total = (long)B * T * 129;
    for (long p = (long)blockIdx.x * NT + threadIdx.x; p < total; p += (long)gridDim.x * NT) {
        const int j = (int)(p % 129);
        const long bt = p / 129;
        const int t = (int)(bt % T), b = (int)(bt / T);
        const float* x = spec + (long)b * sb + (long)t * st;
        const float* d = dout + (long)b * ob + (long)t * ot;
        float g0 = 0.f, g1 = 0.f;
        if (j < 65) {
            const float re = x[(long)j * sf], im = x[(long)j * sf + 1], dr = d[(long)j * of], di = d[(long)j * of + 1];
            g0 = dr * re + di * im;
            g1 = di * re - dr * im;
        } else {
            for (int i = lo[j - 65]; i < hi[j - 65]; ++i) {
                const float wi = ierb_w[(long)i * 64 + (j - 65)];
                if (wi != 0.f) {
                    const int f = 65 + i;
                    const float re = x[(long)f * sf], im = x[(long)f * sf + 1], dr = d[(long)f * of], di = d[(long)f * of + 1];
                    g0 = fmaf(wi, dr * re + di * im, g0);
                    g1 = fmaf(wi, di * re - dr * im, g1);
                }
            }
        }
        dm[p * 2] = g0; dm[p * 2 + 1] = g1;
    }
}

// ---- the same three kernels for DENSE FRAME-MAJOR spectrograms ((B,T,257,2) contiguous: what k_stft writes and the train
// step passes).  One thread per (b,t,j) cost a 64-bit division by the run-time T per item, strided 4-byte accesses with
// 64-bit address arithmetic, and a long tail -- 65 of a frame's 129 items copy one bin, 64 walk a band of up to 12
// (k_feat 288 us at 1.6 TB/s, k_bs_mask 340 us, k_bs_mask_bwd 456 us at 1.8 TB/s).  Here a workgroup stages FM_NF frames
// in LDS with coalesced 8-byte loads and the band sums read LDS.  Per-element arithmetic and its order are unchanged.
constexpr int FM_NF = 4;
constexpr int FM_BW = 12;       // band weights kept in LDS per row / column of the filterbank (the ERB bands are at most 12 bins wide)
__global__ __launch_bounds__(NT) void k_feat_fm(const float* __restrict__ spec, long nframes, const float* __restrict__ erb_w,
                                               float* __restrict__ eb, int bf, float* __restrict__ eb2, int eb2_bf) {
    __shared__ int lo[64], hi[64];
    __shared__ float2 sX[FM_NF][257];
    __shared__ float sWt[64 * FM_BW];           // the bands' weights from their first non-zero bin on (a band wider than FM_BW: global)
    nz_ranges(erb_w, 64, 192, 192, 1, lo, hi);
    for (int i = threadIdx.x; i < 64 * FM_BW; i += NT) {
        const int j = i / FM_BW, u = i - j * FM_BW, k = lo[j] + u;
        sWt[i] = k < hi[j] ? erb_w[(long)j * 192 + k] : 0.f;
    }
    __syncthreads();
    const long groups = (nframes + FM_NF - 1) / FM_NF;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const long bt0 = grp * FM_NF;
        const int nf = (int)(nframes - bt0 < FM_NF ? nframes - bt0 : FM_NF);
        const float2* src = reinterpret_cast<const float2*>(spec + bt0 * 514);
        for (int i = threadIdx.x; i < nf * 257; i += NT) (&sX[0][0])[i] = src[i];
        __syncthreads();
        for (int i = threadIdx.x; i < nf * 129; i += NT) {
            const int fr = i / 129, j = i - fr * 129;
            const float2* x = sX[fr];
            float m = 0.f, re = 0.f, im = 0.f;
            if (j < 65) {
                re = x[j].x; im = x[j].y;
                m = sqrtf(re * re + im * im + 1e-12f);
            } else {
                const float* w = erb_w + (long)(j - 65) * 192;
                const int l0 = lo[j - 65], h0 = hi[j - 65];
                for (int k = l0; k < h0; ++k) {
                    const float wi = k - l0 < FM_BW ? sWt[(j - 65) * FM_BW + k - l0] : w[k];
                    const float r = x[65 + k].x, q = x[65 + k].y;
                    m = fmaf(wi, sqrtf(r * r + q * q + 1e-12f), m);
                    re = fmaf(wi, r, re);
                    im = fmaf(wi, q, im);
                }
            }
            const long p = bt0 * 129 + i;
            sst1(eb, p * 3, bf, m); sst1(eb, p * 3 + 1, bf, re); sst1(eb, p * 3 + 2, bf, im);
            if (eb2) { sst1(eb2, p * 3, eb2_bf, m); sst1(eb2, p * 3 + 1, eb2_bf, re); sst1(eb2, p * 3 + 2, eb2_bf, im); }
        }
        __syncthreads();
    }
}
__global__ __launch_bounds__(NT) void k_bs_mask_fm(const float* __restrict__ m, const float* __restrict__ spec, long nframes,
                                                  const float* __restrict__ ierb_w, float* __restrict__ out, int bf) {
    __shared__ int lo[192], hi[192];
    __shared__ float2 sM[FM_NF][129];
    __shared__ float sWt[192 * 4];              // a bin's band weights from its first non-zero band on (more than 4: global)
    nz_ranges(ierb_w, 192, 64, 64, 1, lo, hi);
    for (int i = threadIdx.x; i < 192 * 4; i += NT) {
        const int f = i >> 2, u = i & 3, j = lo[f] + u;
        sWt[i] = j < hi[f] ? ierb_w[(long)f * 64 + j] : 0.f;
    }
    __syncthreads();
    const long groups = (nframes + FM_NF - 1) / FM_NF;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const long bt0 = grp * FM_NF;
        const int nf = (int)(nframes - bt0 < FM_NF ? nframes - bt0 : FM_NF);
        for (int i = threadIdx.x; i < nf * 129; i += NT) {
            const long e = (bt0 * 129 + i) * 2;
            (&sM[0][0])[i] = make_float2(sld1(m, e, bf), sld1(m, e + 1, bf));
        }
        __syncthreads();
        const float2* xs = reinterpret_cast<const float2*>(spec + bt0 * 514);
        float2* os = reinterpret_cast<float2*>(out + bt0 * 514);
        for (int i = threadIdx.x; i < nf * 257; i += NT) {
            const int fr = i / 257, f = i - fr * 257;
            float m0 = 0.f, m1 = 0.f;
            if (f < 65) {
                m0 = sM[fr][f].x; m1 = sM[fr][f].y;
            } else {
                const float* w = ierb_w + (long)(f - 65) * 64;
                const int l0 = lo[f - 65];
                for (int j = l0; j < hi[f - 65]; ++j) {
                    const float wj = j - l0 < 4 ? sWt[(f - 65) * 4 + j - l0] : w[j];
                    if (wj != 0.f) {
                        m0 = fmaf(wj, sM[fr][65 + j].x, m0);
                        m1 = fmaf(wj, sM[fr][65 + j].y, m1);
                    }
                }
            }
            const float2 x = xs[i];
            os[i] = make_float2(x.x * m0 - x.y * m1, x.y * m0 + x.x * m1);
        }
        __syncthreads();
    }
}
__global__ __launch_bounds__(NT) void k_bs_mask_bwd_fm(const float* __restrict__ dout, const float* __restrict__ spec,
                                                      long nframes, const float* __restrict__ ierb_w, float* __restrict__ dm) {
    __shared__ int lo[64], hi[64];
    __shared__ float2 sG[FM_NF][257];          // per bin: (dr re + di im, di re - dr im)
    __shared__ float sWt[64 * FM_BW];           // a band's column of the (192, 64) matrix from its first non-zero bin on
    nz_ranges(ierb_w, 64, 192, 1, 64, lo, hi);        // columns of the (192, 64) matrix
    for (int i = threadIdx.x; i < 64 * FM_BW; i += NT) {
        const int j = i / FM_BW, u = i - j * FM_BW, k = lo[j] + u;
        sWt[i] = k < hi[j] ? ierb_w[(long)k * 64 + j] : 0.f;
    }
    __syncthreads();
    const long groups = (nframes + FM_NF - 1) / FM_NF;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const long bt0 = grp * FM_NF;
        const int nf = (int)(nframes - bt0 < FM_NF ? nframes - bt0 : FM_NF);
        const float2* xs = reinterpret_cast<const float2*>(spec + bt0 * 514);
        const float2* ds = reinterpret_cast<const float2*>(dout + bt0 * 514);
        for (int i = threadIdx.x; i < nf * 257; i += NT) {
            const float2 x = xs[i], d = ds[i];
            const float re = x.x, im = x.y, dr = d.x, di = d.y;
            (&sG[0][0])[i] = make_float2(dr * re + di * im, di * re - dr * im);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < nf * 129; i += NT) {
            const int fr = i / 129, j = i - fr * 129;
            float g0 = 0.f, g1 = 0.f;
            if (j < 65) {
                g0 = sG[fr][j].x; g1 = sG[fr][j].y;
            } else {
                const int l0 = lo[j - 65];
                for (int k = l0; k < hi[j - 65]; ++k) {
                    const float wi = k - l0 < FM_BW ? sWt[(j - 65) * FM_BW + k - l0] : ierb_w[(long)k * 64 + (j - 65)];
                    if (wi != 0.f) {
                        g0 = fmaf(wi, sG[fr][65 + k].x, g0);
                        g1 = fmaf(wi, sG[fr][65 + k].y, g1);
                    }
                }
            }
            reinterpret_cast<float2*>(dm)[bt0 * 129 + i] = make_float2(g0, g1);
        }
        __syncthreads();
    }
}

// ---- the two thin transposed (1,5) stride-2 convs at the network's edges, 16 -> CO channels, 65 -> 129 bins: decoder.de_convs.4
// forward (CO = 2) and the data gradient of encoder.en_convs.0 (CO = 3).  k_conv<16, CO> gives a thread one output position:
// 64-byte loads at a 64-byte lane stride, and -- the expensive part -- neighbouring lanes have opposite output parity, so a
// wave walks all five taps with half its lanes masked (even bins see kf = 0, 2, 4, odd bins kf = 1, 3): 305 / 314 us.
// Here a workgroup stages four input rows in LDS with coalesced 16-byte loads (records 20 floats apart) and its threads take
// the rows' EVEN bins first, then the odd ones: a wave has one parity, runs only its own taps, and reads the records and the
// tap's weights as 16-byte LDS quads.  Same fmaf chain per output as k_conv (bias - shift first, taps kf ascending, input
// channels ascending): bit-identical outputs.
template <int CO, int FIN, int OUTF>
__global__ __launch_bounds__(NT) void k_thin_tr_fm(long nrows, int w_co, int w_ci, const float* __restrict__ in,
                                                  const float* __restrict__ w, const float* __restrict__ bias,
                                                  const float* __restrict__ shift, float* __restrict__ out) {
    constexpr int NF = 4, PITCH = 20;
    __shared__ __attribute__((aligned(16))) float sX[NF * 65 * PITCH];
    __shared__ __attribute__((aligned(16))) float sWt[5 * 16 * CO];          // [kf][ci][co]
    for (int i = threadIdx.x; i < 5 * 16 * CO; i += NT) {
        const int k = i / (16 * CO), r = i - k * 16 * CO, ci = r / CO, co = r - ci * CO;
        sWt[i] = w[co * w_co + ci * w_ci + k];
    }
    float bv[CO];
#pragma unroll
    for (int co = 0; co < CO; ++co) bv[co] = (bias ? bias[co] : 0.f) - (shift ? shift[co] : 0.f);
    const long groups = (nrows + NF - 1) / NF;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const long r0 = grp * NF;
        const int nf = (int)(nrows - r0 < NF ? nrows - r0 : NF);
        __syncthreads();                                         // (the previous group's reads of sX / the weight table)
        for (int i = threadIdx.x; i < nf * 65 * 4; i += NT) {
            const int pos = i >> 2, q = i & 3;
            *reinterpret_cast<f32x4*>(sX + pos * PITCH + 4 * q) = sld4<kNt>(in, (r0 * 65 + pos) * 16 + 4 * q, FIN);
        }
        __syncthreads();
        const int nE = nf * 65;                                  // even bins 0, 2 .. 128 of the rows, then the odd ones
        for (int i = threadIdx.x; i < nf * 129; i += NT) {
            const bool odd = i >= nE;
            const int ii = odd ? i - nE : i, per = odd ? 64 : 65, fr = ii / per, j = ii - fr * per, fo = 2 * j + (odd ? 1 : 0);
            float acc[CO];
#pragma unroll
            for (int co = 0; co < CO; ++co) acc[co] = bv[co];
            // even: taps 0, 2, 4 read bins j + 1, j, j - 1; odd: taps 1, 3 read bins j + 1, j
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int fi = j + 1 - u, k = odd ? 2 * u + 1 : 2 * u;
                if (fi < 0 || fi >= 65 || (odd && u == 2)) continue;
                const f32x4* xq = reinterpret_cast<const f32x4*>(sX + (fr * 65 + fi) * PITCH);
                const f32x4* wq = reinterpret_cast<const f32x4*>(sWt + k * 16 * CO);
                float xv[16], wv[16 * CO];
#pragma unroll
                for (int v = 0; v < 4; ++v) { const f32x4 t = xq[v]; xv[4 * v] = t[0]; xv[4 * v + 1] = t[1]; xv[4 * v + 2] = t[2]; xv[4 * v + 3] = t[3]; }
#pragma unroll
                for (int v = 0; v < 4 * CO; ++v) { const f32x4 t = wq[v]; wv[4 * v] = t[0]; wv[4 * v + 1] = t[1]; wv[4 * v + 2] = t[2]; wv[4 * v + 3] = t[3]; }
#pragma unroll
                for (int ci = 0; ci < 16; ++ci)
#pragma unroll
                    for (int co = 0; co < CO; ++co) acc[co] = fmaf(wv[ci * CO + co], xv[ci], acc[co]);
            }
            const long o = ((r0 + fr) * 129 + fo) * CO;
#pragma unroll
            for (int co = 0; co < CO; ++co) sst1(out, o + co, OUTF, acc[co]);
        }
    }
}

// ---- the same three kernels for the layout the callers actually pass: (B,257,T,2) with the FRAME axis fastest
// (torch.stft's, st < sf).  One thread per (b,t,f) with f fastest then reads / writes the 0.5 GB spectrograms 8 bytes
// at a time with a stride of 2 T floats (k_bs_mask_bwd ran at 0.7 TB/s).  Here a workgroup takes a tile of TT frames of
// one utterance: lanes run along t (coalesced rows of the spectrograms), the frame-major side -- m / dm / eb, which
// is CONTIGUOUS for a tile -- goes through LDS.  Per-element arithmetic and its order are unchanged.
constexpr int TT = 32;
__global__ __launch_bounds__(NT) void k_feat_t(const float* __restrict__ spec, long sb, long sf, long st, int B, int T,
                                              const float* __restrict__ erb_w, float* __restrict__ eb, int bf,
                                              float* __restrict__ eb2, int eb2_bf) {
    __shared__ int lo[64], hi[64];
    __shared__ float tile[TT][129 * 3 + 1];
    nz_ranges(erb_w, 64, 192, 192, 1, lo, hi);
    const int tiles = (T + TT - 1) / TT;
    const int b = blockIdx.x / tiles, t0 = (blockIdx.x - b * tiles) * TT, nt = min(TT, T - t0);
    const int tl = threadIdx.x & (TT - 1), r = threadIdx.x / TT;
    if (tl < nt) {
        const float* x = spec + (long)b * sb + (long)(t0 + tl) * st;
        for (int j = r; j < 129; j += NT / TT) {
            float m = 0.f, re = 0.f, im = 0.f;
            if (j < 65) {
                re = x[(long)j * sf]; im = x[(long)j * sf + 1];
                m = sqrtf(re * re + im * im + 1e-12f);
            } else {
                // a band's bins are requested TOGETHER (up to BW; a band of the shipped bank has at most 11), then the
                // multiply-adds in ascending-bin order: one bin per trip behind `if (w != 0)` was a chain of dependent
                // round trips (415 us at 1.4 TB/s).  Bins past the band's end load a valid bin and meet a zero weight
                // (m + 0 * x: the same value for finite input, and what the reference's dense matmul computes).
                constexpr int BW = 12;
                const float* w = erb_w + (long)(j - 65) * 192;
                const int l0 = lo[j - 65], h0 = hi[j - 65];
                float2 xv[BW];
                float wv[BW];
#pragma unroll
                for (int u = 0; u < BW; ++u) {
                    const int i = l0 + u < 192 ? l0 + u : 191;
                    xv[u] = *reinterpret_cast<const float2*>(x + (long)(65 + i) * sf);
                    wv[u] = l0 + u < h0 ? w[i] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < BW; ++u) {
                    const float rr = xv[u].x, q = xv[u].y;
                    m = fmaf(wv[u], sqrtf(rr * rr + q * q + 1e-12f), m);
                    re = fmaf(wv[u], rr, re);
                    im = fmaf(wv[u], q, im);
                }
                for (int i = l0 + BW; i < h0; ++i) {              // (a wider band of some other bank)
                    const float wi = w[i];
                    const float rr = x[(long)(65 + i) * sf], q = x[(long)(65 + i) * sf + 1];
                    m = fmaf(wi, sqrtf(rr * rr + q * q + 1e-12f), m);
                    re = fmaf(wi, rr, re);
                    im = fmaf(wi, q, im);
                }
            }
            tile[tl][j * 3] = m; tile[tl][j * 3 + 1] = re; tile[tl][j * 3 + 2] = im;
        }
    }
    __syncthreads();
    const long base = ((long)b * T + t0) * 387;
    for (int i = threadIdx.x; i < nt * 387; i += NT) {
        sst1(eb, base + i, bf, tile[i / 387][i % 387]);
        if (eb2) sst1(eb2, base + i, eb2_bf, tile[i / 387][i % 387]);
    }
}

__global__ __launch_bounds__(NT) void k_bs_mask_t(const float* __restrict__ m, const float* __restrict__ spec, long sb,
                                                 long sf, long st, int B, int T, const float* __restrict__ ierb_w,
                                                 float* __restrict__ out, long ob, long of, long ot, int bf) {
    __shared__ int lo[192], hi[192];
    __shared__ float sm[TT][258 + 2];
    nz_ranges(ierb_w, 192, 64, 64, 1, lo, hi);
    const int tiles = (T + TT - 1) / TT;
    const int b = blockIdx.x / tiles, t0 = (blockIdx.x - b * tiles) * TT, nt = min(TT, T - t0);
    const long mbase = ((long)b * T + t0) * 258;
    for (int i = threadIdx.x; i < nt * 258; i += NT) sm[i / 258][i % 258] = sld1(m, mbase + i, bf);
    __syncthreads();
    const int tl = threadIdx.x & (TT - 1), r = threadIdx.x / TT;
    if (tl >= nt) return;
    const float* xr = spec + (long)b * sb + (long)(t0 + tl) * st;
    float* orow = out + (long)b * ob + (long)(t0 + tl) * ot;
    const float* mt = sm[tl];
    // (the spectrogram values of eight of the thread's bins are requested together: one bin per trip was 33 dependent
    // round trips per thread)
    constexpr int RS_ = NT / TT, UB = 8;
    for (int f0 = r; f0 < 257; f0 += UB * RS_) {
        float2 xv[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int f = f0 + u * RS_;
            xv[u] = *reinterpret_cast<const float2*>(xr + (long)(f < 257 ? f : 0) * sf);
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int f = f0 + u * RS_;
            if (f >= 257) break;
            float m0 = 0.f, m1 = 0.f;
            if (f < 65) {
                m0 = mt[f * 2]; m1 = mt[f * 2 + 1];
            } else {
                const float* w = ierb_w + (long)(f - 65) * 64;
                for (int j = lo[f - 65]; j < hi[f - 65]; ++j) {
                    const float wj = w[j];
                    if (wj != 0.f) {
                        m0 = fmaf(wj, mt[(65 + j) * 2], m0);
                        m1 = fmaf(wj, mt[(65 + j) * 2 + 1], m1);
                    }
                }
            }
            float* o = orow + (long)f * of;
            *reinterpret_cast<float2*>(o) = make_float2(xv[u].x * m0 - xv[u].y * m1, xv[u].y * m0 + xv[u].x * m1);
        }
    }
}

__global__ __launch_bounds__(NT) void k_bs_mask_bwd_t(const float* __restrict__ dout, long ob, long of, long ot,
                                                     const float* __restrict__ spec, long sb, long sf, long st, int B,
                                                     int T, const float* __restrict__ ierb_w, float* __restrict__ dm) {
    __shared__ int lo[64], hi[64];
    __shared__ float sd[TT][258 + 2];
    nz_ranges(ierb_w, 64, 192, 1, 64, lo, hi);        // columns of the (192, 64) matrix
    const int tiles = (T + TT - 1) / TT;
    const int b = blockIdx.x / tiles, t0 = (blockIdx.x - b * tiles) * TT, nt = min(TT, T - t0);
    const int tl = threadIdx.x & (TT - 1), r = threadIdx.x / TT;
    if (tl < nt) {
        const float* x = spec + (long)b * sb + (long)(t0 + tl) * st;
        const float* d = dout + (long)b * ob + (long)(t0 + tl) * ot;
        for (int j = r; j < 129; j += NT / TT) {
            float g0 = 0.f, g1 = 0.f;
            if (j < 65) {
                const float re = x[(long)j * sf], im = x[(long)j * sf + 1], dr = d[(long)j * of], di = d[(long)j * of + 1];
                g0 = dr * re + di * im;
                g1 = di * re - dr * im;
            } else {
                constexpr int BW = 12;                              // (see k_feat_t)
                const int l0 = lo[j - 65], h0 = hi[j - 65];
                float2 xv[BW], dv[BW];
                float wv[BW];
#pragma unroll
                for (int u = 0; u < BW; ++u) {
                    const int i = l0 + u < 192 ? l0 + u : 191;
                    xv[u] = *reinterpret_cast<const float2*>(x + (long)(65 + i) * sf);
                    dv[u] = *reinterpret_cast<const float2*>(d + (long)(65 + i) * of);
                    wv[u] = l0 + u < h0 ? ierb_w[(long)i * 64 + (j - 65)] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < BW; ++u) {
                    g0 = fmaf(wv[u], dv[u].x * xv[u].x + dv[u].y * xv[u].y, g0);
                    g1 = fmaf(wv[u], dv[u].y * xv[u].x - dv[u].x * xv[u].y, g1);
                }
                for (int i = l0 + BW; i < h0; ++i) {
                    const float wi = ierb_w[(long)i * 64 + (j - 65)];
                    const int f = 65 + i;
                    const float re = x[(long)f * sf], im = x[(long)f * sf + 1], dr = d[(long)f * of], di = d[(long)f * of + 1];
                    g0 = fmaf(wi, dr * re + di * im, g0);
                    g1 = fmaf(wi, di * re - dr * im, g1);
                }
            }
            sd[tl][j * 2] = g0; sd[tl][j * 2 + 1] = g1;
        }
    }
    __syncthreads();
    const long base = ((long)b * T + t0) * 258;
    for (int i = threadIdx.x; i < nt * 258; i += NT) dm[base + i] = sd[i / 258][i % 258];
}

// ---------------------------------------------------------------------------------- TRALite
// point_bn2 on load (fusion bit 12): TRALite's input v is point_bn2(point_conv2(.)) with NO activation behind it
// (models/gtcrn_micro.py:222-223, 248), read by four kernels -- energy, gate/shuffle and their two backward passes.  With
// bn.stats != nullptr they take point_conv2's conv output y (format bn.ybf) instead and normalise it themselves: k_bn_act's
// expression, rounded to the activations' storage format bf exactly as the stored activation was, so every value is the
// one the separate pass (read y, write v: six launches per step) produced, bit for bit -- and v is never stored.
struct BnLoad { const float *stats, *gamma, *beta; int ybf; };
struct BnLoad4 { f32x4 mean, istd, gm, bt; };
__device__ __forceinline__ BnLoad4 bnl_const(const BnLoad& b, int c0) {     // channels c0 .. c0 + 3 of 8
    BnLoad4 k{};
    if (b.stats) {
        k.mean = *reinterpret_cast<const f32x4*>(b.stats + c0); k.istd = *reinterpret_cast<const f32x4*>(b.stats + 8 + c0);
        k.gm = *reinterpret_cast<const f32x4*>(b.gamma + c0); k.bt = *reinterpret_cast<const f32x4*>(b.beta + c0);
    }
    return k;
}
__device__ __forceinline__ float bnl_apply1(float y, float mean, float istd, float gm, float bt, int bf) {
    return round16(gm * ((y - mean) * istd) + bt, bf);
}
template <bool NTL>
__device__ __forceinline__ f32x4 bnl_ld4(const BnLoad& b, const BnLoad4& k, const float* v, long idx, int bf) {
    if (!b.stats) return sld4<NTL>(v, idx, bf);
    const f32x4 y = sld4<NTL>(v, idx, b.ybf);
    f32x4 a;
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = bnl_apply1(y[e], k.mean[e], k.istd[e], k.gm[e], k.bt[e], bf);
    return a;
}
// TRALite.forward (models/gtcrn_micro.py:122-139) with a zero cache: e = mean_F(v^2); y = causal depthwise
// conv1d (k=3, bias) over [0,0 | e]; g = sigmoid(point_conv(y)).  v: [B][Tt][33][8].
__global__ __launch_bounds__(NT) void k_tra_energy(const float* __restrict__ v, long rows, float* __restrict__ e,
                                                  int bf, BnLoad bn) {
    const int c_ = threadIdx.x & 7;                   // (the grid stride is a multiple of 8: a thread's channel is fixed)
    const float mean = bn.stats ? bn.stats[c_] : 0.f, istd = bn.stats ? bn.stats[8 + c_] : 0.f;
    const float gm = bn.stats ? bn.gamma[c_] : 0.f, bt = bn.stats ? bn.beta[c_] : 0.f;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < rows * 8; i += (long)gridDim.x * NT) {
        const int c = (int)(i & 7);
        const long p = (i >> 3) * 33 * 8 + c;
        float s = 0.f;
        if (bn.stats) {
            for (int f = 0; f < 33; ++f) {
                const float x = bnl_apply1(sld1(v, p + f * 8, bn.ybf), mean, istd, gm, bt, bf);
                s = fmaf(x, x, s);
            }
        } else
        for (int f = 0; f < 33; ++f) { const float x = sld1(v, p + f * 8, bf); s = fmaf(x, x, s); }
        e[i] = s * (1.0f / 33.0f);
    }
}
__global__ __launch_bounds__(NT) void k_tra_gate(const float* __restrict__ e, int B, int Tt,
                                                const float* __restrict__ dw_w, const float* __restrict__ dw_b,
                                                const float* __restrict__ pw_w, const float* __restrict__ pw_b,
                                                float* __restrict__ y, float* __restrict__ g) {
    const long total = (long)B * Tt * 8;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int co = (int)(i & 7);
        const long row = i >> 3;
        const int t = (int)(row % Tt);
        float z = pw_b[co];
        for (int c = 0; c < 8; ++c) {
            float yc = dw_b[c];
            for (int k = 0; k < 3; ++k) {
                const int tt = t - 2 + k;
                if (tt >= 0) yc = fmaf(dw_w[c * 3 + k], e[(row - 2 + k) * 8 + c], yc);
            }
            if (c == co) y[i] = yc;
            z = fmaf(pw_w[co * 8 + c], yc, z);
        }
        g[i] = 1.0f / (1.0f + expf(-z));
    }
}
// TRA gate + channel shuffle (:222-227, :246-253): out[2c] = v[c] * g[c], out[2c+1] = x2[c] = x[8+c]
__global__ __launch_bounds__(NT) void k_gate_shuffle(const float* __restrict__ v, const float* __restrict__ g,
                                                    const float* __restrict__ x, int B, int T, int Tt,
                                                    float* __restrict__ out, int bf, float* __restrict__ out2,
                                                    int out2_bf, const float* __restrict__ skip, BnLoad bn) {
    // thread (position, half h): channels 4h..4h+3 -> output slots 8h..8h+7; 16-byte accesses throughout
    // skip (optional, format bf): out = block output + skip, the next decoder layer's input (Decoder.forward,
    // models/gtcrn_micro.py:463-469: x = de_convs[i](x + en_outs[4 - i])) -- the block output has no other reader
    const long total = (long)B * T * 33 * 2;
    const BnLoad4 bk = bnl_const(bn, 4 * (threadIdx.x & 1));      // (even grid stride: a thread's half h is fixed)
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int h = (int)(i & 1);
        const long pos = i >> 1;                      // (b, t, f) over T frames
        const int f = (int)(pos % 33);
        const long bt = pos / 33;
        const int t = (int)(bt % T), b = (int)(bt / T);
        const long rowv = (long)b * Tt + t;
        const f32x4 vv = bnl_ld4<kNt>(bn, bk, v, (rowv * 33 + f) * 8 + 4 * h, bf);
        const f32x4 gg = *reinterpret_cast<const f32x4*>(g + rowv * 8 + 4 * h);
        const f32x4 xx = sld4(x, pos * 16 + 8 + 4 * h, bf);
        const f32x4 p = vv * gg;
        if (skip) {
            const f32x4 k0 = sld4<kNt>(skip, pos * 16 + 8 * h, bf), k1 = sld4<kNt>(skip, pos * 16 + 8 * h + 4, bf);
            // (16-bit storage: the block output rounded as the stored one was, then the same add as the separate pass)
            sst4<kNtSt>(out, pos * 16 + 8 * h, bf, round_bf4(f32x4{p[0], xx[0], p[1], xx[1]}, bf) + k0);
            sst4<kNtSt>(out, pos * 16 + 8 * h + 4, bf, round_bf4(f32x4{p[2], xx[2], p[3], xx[3]}, bf) + k1);
            continue;
        }
        sst4<kNtSt>(out, pos * 16 + 8 * h, bf, f32x4{p[0], xx[0], p[1], xx[1]});
        sst4<kNtSt>(out, pos * 16 + 8 * h + 4, bf, f32x4{p[2], xx[2], p[3], xx[3]});
        if (out2) {
            sst4<kNtSt>(out2, pos * 16 + 8 * h, out2_bf, f32x4{p[0], xx[0], p[1], xx[1]});
            sst4<kNtSt>(out2, pos * 16 + 8 * h + 4, out2_bf, f32x4{p[2], xx[2], p[3], xx[3]});
        }
    }
}
// backward, last step (after k_tra_dgate / k_tra_dy): dv = dout[2c] * g (0 on the trimmed tail frames) + de * (2/33) * v
// with de[t][c] = sum_k dw[c][k] * dy[t + 2 - k][c] (the energy path of TRALite), dx[8+c] = dout[2c+1].  One pass: the
// gate path used to be stored first and the energy path added by a read-modify-write pass of its own (k_tra_dv,
// 146 us per block).  Same expression, fmaf(de, v, dout * g), as the two passes.
__global__ __launch_bounds__(NT) void k_gate_shuffle_bwd(const float* __restrict__ dout, const float* __restrict__ g,
                                                        const float* __restrict__ dy, const float* __restrict__ v,
                                                        const float* __restrict__ dw_w, int B, int T, int Tt,
                                                        float* __restrict__ dv, float* __restrict__ dx, int bf,
                                                        int dx_acc, BnLoad bn, int gbf) {
    // thread (position of the T' frames, half h): channels 4h..4h+3; 16-byte accesses.  dx_acc: the pass-through half
    // is ADDED to what dx holds (the skip gradient of the same tensor, see gtcrn_train_backward)
    const long total = (long)B * Tt * 33 * 2;
    const BnLoad4 bk = bnl_const(bn, 4 * (threadIdx.x & 1));
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int h = (int)(i & 1);
        const long posv = i >> 1;
        const int f = (int)(posv % 33);
        const long rowv = posv / 33;
        const int t = (int)(rowv % Tt), b = (int)(rowv / Tt);
        f32x4 r = {0.f, 0.f, 0.f, 0.f};
        if (t < T) {
            const long pos = ((long)b * T + t) * 33 + f;
            const f32x4 d0 = sld4<kNt>(dout, pos * 16 + 8 * h, gbf), d1 = sld4<kNt>(dout, pos * 16 + 8 * h + 4, gbf);   // gbf: format of dout / dx / dv
            const f32x4 gg = *reinterpret_cast<const f32x4*>(g + rowv * 8 + 4 * h);
            r = f32x4{d0[0], d0[2], d1[0], d1[2]} * gg;
            f32x4 px = f32x4{d0[1], d0[3], d1[1], d1[3]};
            if (dx_acc) px = px + sld4(dx, pos * 16 + 8 + 4 * h, gbf);
            sst4(dx, pos * 16 + 8 + 4 * h, gbf, px);
        }
        f32x4 de = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < 3; ++k) {
            const int tt = t + 2 - k;
            if (tt < Tt) {
                const f32x4 dyv = *reinterpret_cast<const f32x4*>(dy + (rowv + 2 - k) * 8 + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) de[e] = fmaf(dw_w[(4 * h + e) * 3 + k], dyv[e], de[e]);
            }
        }
        const f32x4 vv = bnl_ld4<kNt>(bn, bk, v, posv * 8 + 4 * h, bf);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaf(de[e] * (2.0f / 33.0f), vv[e], r[e]);
        sst4<kNtSt>(dv, posv * 8 + 4 * h, gbf, o);
    }
}
// step 2: dg = sum_F dout[2c] * v  ->  dzg = dg * g * (1 - g)
__global__ __launch_bounds__(NT) void k_tra_dgate(const float* __restrict__ dout, const float* __restrict__ v,
                                                 const float* __restrict__ g, int B, int T, int Tt,
                                                 float* __restrict__ dzg, int bf, BnLoad bn, int gbf) {
    // one wave per row (b, t): lane (position, quad q) takes dout slots 4q..4q+3 = channels 2q, 2q+1 (16-byte loads;
    // one thread per (row, channel) walked the 33 bins with 4-byte loads at a 64-byte stride), then the lanes of a
    // quad are summed by xor shuffles
    const long rows = (long)B * Tt;
    const int lane = threadIdx.x & 63, q = lane & 3;
    float bm[2] = {0.f, 0.f}, bi[2] = {0.f, 0.f}, bg[2] = {0.f, 0.f}, bb[2] = {0.f, 0.f};   // channels 2q, 2q + 1
    if (bn.stats)
        for (int e = 0; e < 2; ++e) {
            bm[e] = bn.stats[2 * q + e]; bi[e] = bn.stats[8 + 2 * q + e]; bg[e] = bn.gamma[2 * q + e]; bb[e] = bn.beta[2 * q + e];
        }
    const long nw = (long)gridDim.x * (NT / 64);
    for (long rowv = (long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6); rowv < rows; rowv += nw) {
        const int t = (int)(rowv % Tt), b = (int)(rowv / Tt);
        float s0 = 0.f, s1 = 0.f;
        if (t < T) {
            const long dbase = (((long)b * T + t) * 33) * 16, vbase = rowv * 33 * 8;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int it = lane + 64 * k;
                if (it < 132) {
                    const int pos = it >> 2;
                    const f32x4 d = sld4(dout, dbase + pos * 16 + 4 * q, gbf);
                    if (bn.stats) {
                        s0 = fmaf(d[0], bnl_apply1(sld1(v, vbase + pos * 8 + 2 * q, bn.ybf), bm[0], bi[0], bg[0], bb[0], bf), s0);
                        s1 = fmaf(d[2], bnl_apply1(sld1(v, vbase + pos * 8 + 2 * q + 1, bn.ybf), bm[1], bi[1], bg[1], bb[1], bf), s1);
                    } else {
                        s0 = fmaf(d[0], sld1(v, vbase + pos * 8 + 2 * q, bf), s0);
                        s1 = fmaf(d[2], sld1(v, vbase + pos * 8 + 2 * q + 1, bf), s1);
                    }
                }
            }
        }
#pragma unroll
        for (int off = 32; off >= 4; off >>= 1) { s0 += __shfl_xor(s0, off, 64); s1 += __shfl_xor(s1, off, 64); }
        if (lane < 4) {
            const float g0 = g[rowv * 8 + 2 * q], g1 = g[rowv * 8 + 2 * q + 1];
            dzg[rowv * 8 + 2 * q] = s0 * g0 * (1.f - g0);
            dzg[rowv * 8 + 2 * q + 1] = s1 * g1 * (1.f - g1);
        }
    }
}
// step 3: dy[c] = sum_co pw[co][c] * dzg[co]
__global__ __launch_bounds__(NT) void k_tra_dy(const float* __restrict__ dzg, long rows, const float* __restrict__ pw_w,
                                              float* __restrict__ dy) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < rows * 8; i += (long)gridDim.x * NT) {
        const int c = (int)(i & 7);
        const float* d = dzg + (i >> 3) * 8;
        float s = 0.f;
        for (int co = 0; co < 8; ++co) s = fmaf(pw_w[co * 8 + c], d[co], s);
        dy[i] = s;
    }
}
// parameter gradients of the two conv1d: 104 sums over the rows (b,t), per-workgroup partials, in the order
// the blob stores them: [0,24) d dw_w[c][k] = sum dy[t][c] * e[t-2+k][c]   [24,32) d dw_b[c] = sum dy[c]
//                       [32,96) d pw_w[co][c] = sum dzg[co] * y[c]         [96,104) d pw_b[co] = sum dzg[co]
// (1024 threads = 8 row slices x 128: with one 128-thread slice per workgroup the ~127 rows of a workgroup were a serial
// chain of dependent-latency loads, 107 us for 16 MB of input)
__global__ __launch_bounds__(1024) void k_tra_pgrad(const float* __restrict__ dzg, const float* __restrict__ y,
                                                   const float* __restrict__ dy, const float* __restrict__ e, int B,
                                                   int Tt, float* __restrict__ partial) {
    __shared__ float sh[8][104];
    const int tid = threadIdx.x & 127, slice = threadIdx.x >> 7;
    const long rows = (long)B * Tt;
    const long per = (rows + gridDim.x - 1) / gridDim.x;
    const long r0 = (long)blockIdx.x * per, r1 = r0 + per < rows ? r0 + per : rows;
    float s = 0.f;
    if (tid < 104) {
        // a thread's role is fixed: operand pointers and the frame offset of the second one once, then the rows FOUR at a
        // time -- all eight loads requested before the first multiply-add (one row per trip was a chain of ~16 dependent
        // load latencies per thread: 47 us for 17 MB of input); same order of additions as the row-by-row loop
        const float* pa;
        const float* pb = nullptr;
        int back = 0;                       // rows the second operand lies behind (the conv1d taps), 0 otherwise
        if (tid < 24) { const int c = tid / 3, k = tid % 3; pa = dy + c; pb = e + c; back = 2 - k; }
        else if (tid < 32) pa = dy + (tid - 24);
        else if (tid < 96) { pa = dzg + ((tid - 32) >> 3); pb = y + ((tid - 32) & 7); }
        else pa = dzg + (tid - 96);
        long r = r0 + slice;
        for (; r + 24 < r1; r += 32) {
            float a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long ru = r + 8 * u;
                const bool ok = (int)(ru % Tt) - back >= 0;
                a[u] = pa[ru * 8];
                b[u] = pb ? (ok ? pb[(ru - back) * 8] : 0.f) : 1.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) s = pb ? fmaf(a[u], b[u], s) : s + a[u];
        }
        for (; r < r1; r += 8) {
            const bool ok = (int)(r % Tt) - back >= 0;
            const float a = pa[r * 8];
            if (pb) { if (ok) s = fmaf(a, pb[(r - back) * 8], s); }
            else s += a;
        }
        sh[slice][tid] = s;
    }
    __syncthreads();
    if (slice == 0 && tid < 104) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) t += sh[q][tid];
        partial[(long)blockIdx.x * 104 + tid] = t;
    }
}

// ------------------------------------------------------------------------------- HybridLoss
// loss.py:30-71: 30 * (MSE of the power-compressed real and imaginary parts) + 70 * MSE of the compressed
// magnitudes + SI-SNR of the sqrt-Hann iSTFTs.  k_hloss_spec: value and gradient of the three spectral
// terms in one pass over (B,257,T); the SI-SNR term needs three sums per utterance (k_sisnr_sums), from which
// its gradient w.r.t. the predicted waveform is A_b * y_pred + B_b * y_true (k_sisnr_coef, k_sisnr_gwave);
// the iSTFT adjoint (kernels.hip, k_stft<true>) carries it back to the spectrogram.
// FMAJ: the elements are walked bin-fastest (frame-major spectrograms: st > sf), otherwise frame-fastest (torch.stft's layout)
template <bool FMAJ>
__global__ __launch_bounds__(NT) void k_hloss_spec(const float* __restrict__ pred, long pb, long pf, long pt,
                                                  const float* __restrict__ tru, long tb, long tf, long tt, int B,
                                                  int T, float* __restrict__ grad, long gb, long gf, long gt,
                                                  double* __restrict__ partial) {
    __shared__ double sh[NT];
    const long N = (long)B * 257 * T;
    const float kri = 60.0f / (float)N, kmag = 140.0f / (float)N;
    double sri = 0.0, smag = 0.0;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < N; i += (long)gridDim.x * NT) {
        int t, f, b;
        const unsigned iu = (unsigned)i;                 // (N < 2^31: the launcher checks)
        if constexpr (FMAJ) {
            const unsigned bt = iu / 257u, ub = bt / (unsigned)T;
            f = (int)(iu - bt * 257u);
            t = (int)(bt - ub * (unsigned)T); b = (int)ub;
        } else {
            const unsigned bf = iu / (unsigned)T, ub = bf / 257u;
            t = (int)(iu - bf * (unsigned)T);
            f = (int)(bf - ub * 257u); b = (int)ub;
        }
        const float2 p = *reinterpret_cast<const float2*>(pred + (long)b * pb + (long)f * pf + (long)t * pt);
        const float2 q = *reinterpret_cast<const float2*>(tru + (long)b * tb + (long)f * tf + (long)t * tt);
        const float pm2 = p.x * p.x + p.y * p.y + 1e-12f, tm2 = q.x * q.x + q.y * q.y + 1e-12f;
        const float lp = 0.5f * __log2f(pm2), lt = 0.5f * __log2f(tm2);      // log2 |.|
        const float u = exp2f(-0.7f * lp), ut = exp2f(-0.7f * lt);            // |.|^-0.7
        const float c = exp2f(0.3f * lp), ct = exp2f(0.3f * lt);              // |.|^0.3
        const float da = p.x * u - q.x * ut, db = p.y * u - q.y * ut, dc = c - ct;
        sri += (double)(da * da + db * db);
        smag += (double)(dc * dc);
        if (grad) {
            const float inv = 1.0f / pm2, w = 0.7f * u * inv;
            const float a_r = u - w * p.x * p.x, a_i = -w * p.x * p.y, b_i = u - w * p.y * p.y;
            const float cw = 0.3f * c * inv;
            *reinterpret_cast<float2*>(grad + (long)b * gb + (long)f * gf + (long)t * gt) =
                make_float2(kri * (da * a_r + db * a_i) + kmag * dc * cw * p.x,
                            kri * (da * a_i + db * b_i) + kmag * dc * cw * p.y);
        }
    }
    // workgroup sums, fixed order
    for (int k = 0; k < 2; ++k) {
        __syncthreads();
        sh[threadIdx.x] = k == 0 ? sri : smag;
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int j = 0; j < NT; ++j) s += sh[j];
            partial[(long)blockIdx.x * 2 + k] = s;
        }
    }
}
// per utterance: dot = <yt, yp>, ett = <yt, yt>, epp = <yp, yp>; grid (chunks, B).  The products are formed in double,
// where the product of two floats is exact: k_sisnr_coef expands |yp - s|^2 from these three sums, and for a
// prediction close to its target that expansion cancels down to the rounding of the sums (products rounded to float
// first lost the residual from 60 dB SI-SNR on: tests/reports/README.md)
__global__ __launch_bounds__(NT) void k_sisnr_sums(const float* __restrict__ yp, const float* __restrict__ yt, long Lw,
                                                  double* __restrict__ partial) {
    __shared__ double sh[NT];
    const float* a = yp + (long)blockIdx.y * Lw;
    const float* b = yt + (long)blockIdx.y * Lw;
    double v[3] = {0.0, 0.0, 0.0};
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < Lw; i += (long)gridDim.x * NT) {
        const double x = (double)a[i], y = (double)b[i];
        v[0] += x * y; v[1] += y * y; v[2] += x * x;
    }
    for (int k = 0; k < 3; ++k) {
        __syncthreads();
        sh[threadIdx.x] = v[k];
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int j = 0; j < NT; ++j) s += sh[j];
            partial[((long)blockIdx.y * gridDim.x + blockIdx.x) * 3 + k] = s;
        }
    }
}
// one thread per utterance: -log10(|s|^2 / (|yp - s|^2 + 1e-8) + 1e-8) with s = <yt,yp> yt / (<yt,yt> + 1e-8), and the
// coefficients of its gradient  d/d yp = A yp + B yt  (scaled by 1/B: the loss takes the batch mean).
// Thread 0 of block 0 also closes the loss: spectral partial sums + mean SI-SNR.
__global__ void k_sisnr_coef(const double* __restrict__ part, int chunks, int B, long N,
                             const double* __restrict__ spec_partial, int spec_parts, float* __restrict__ coef,
                             double* __restrict__ vals, float* __restrict__ loss) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) {
        double dot = 0.0, ett = 0.0, epp = 0.0;
        for (int c = 0; c < chunks; ++c) {
            dot += part[((long)b * chunks + c) * 3]; ett += part[((long)b * chunks + c) * 3 + 1];
            epp += part[((long)b * chunks + c) * 3 + 2];
        }
        const double eps = 1e-8, al = dot / (ett + eps), num = al * al * ett;
        const double den = epp - 2.0 * al * dot + al * al * ett + eps;
        const double r = num / den;
        vals[b] = -log10(r + eps);
        const double c0 = (1.0 / B) * (-1.0 / ((r + eps) * 2.302585092994046));
        const double kap = ett / (ett + eps), eta = (dot - al * ett) / (ett + eps);
        coef[2 * b] = (float)(c0 * (-2.0 * num / (den * den)));
        coef[2 * b + 1] = (float)(c0 * (2.0 * al * kap / den + 2.0 * num * (al + eta) / (den * den)));
    }
    // the last step needs every utterance's value: a single-block launch keeps it simple (B <= 1024 per block).  Every
    // thread takes a strided share of the spectral partials and its own utterance's value, then a fixed-order tree in LDS
    // (one thread walking ~2 500 values one dependent load at a time took 157 us of every step)
    if (gridDim.x != 1) return;
    __shared__ double sh[3][1024];
    const int t = threadIdx.x, nth = blockDim.x;
    double sri = 0.0, smag = 0.0;
    for (int w = t; w < spec_parts; w += nth) { sri += spec_partial[2 * w]; smag += spec_partial[2 * w + 1]; }
    sh[0][t] = sri; sh[1][t] = smag; sh[2][t] = b < B ? vals[b] : 0.0;       // (vals[b]: this thread's own store above)
    __syncthreads();
    for (int h = nth >> 1; h >= 1; h >>= 1) {                                 // (nth is a power of two: 1024)
        if (t < h) { sh[0][t] += sh[0][t + h]; sh[1][t] += sh[1][t + h]; sh[2][t] += sh[2][t + h]; }
        __syncthreads();
    }
    if (t == 0) loss[0] = (float)(30.0 * sh[0][0] / (double)N + 70.0 * sh[1][0] / (double)N + sh[2][0] / B);
}
// gwave = (A_b yp + B_b yt) / envelope, envelope[j] = win[j & 255]^2 + win[256 + (j & 255)]^2 (k_istft divides by it)
__global__ __launch_bounds__(NT) void k_sisnr_gwave(float* __restrict__ yp, const float* __restrict__ yt, long Lw,
                                                   long total, const float* __restrict__ coef,
                                                   const float* __restrict__ win) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int b = (int)(i / Lw), j = (int)((i - (long)b * Lw) & 255);
        const float env = win[j] * win[j] + win[256 + j] * win[256 + j];
        const float g = coef[2 * b] * yp[i] + coef[2 * b + 1] * yt[i];
        yp[i] = env > 1e-11f ? g / env : g;
    }
}

__global__ __launch_bounds__(NT) void k_add(const float* __restrict__ a, const float* __restrict__ b,
                                           float* __restrict__ out, long n) {
    if ((n & 3) == 0 && ((reinterpret_cast<size_t>(a) | reinterpret_cast<size_t>(b) | reinterpret_cast<size_t>(out)) & 15) == 0) {
        // (every tensor of the model: 16-byte accesses)
        for (long i = (long)blockIdx.x * NT + threadIdx.x; i < (n >> 2); i += (long)gridDim.x * NT)
            sst4<kNtSt>(out, 4 * i, 0, sld4<kNt>(a, 4 * i, 0) + sld4<kNt>(b, 4 * i, 0));
        return;
    }
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) out[i] = a[i] + b[i];
}

// forward sums of saved tensors (decoder: x + skip), vector of 4
__global__ __launch_bounds__(NT) void k_add_saved(const float* __restrict__ a, const float* __restrict__ b,
                                                 float* __restrict__ out, long n4, int bf) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long)gridDim.x * NT)
        sst4<kNtSt>(out, i * 4, bf, sld4<kNt>(a, i * 4, bf) + sld4<kNt>(b, i * 4, bf));
}
__global__ __launch_bounds__(NT) void k_saved_to_f32(const float* __restrict__ src, float* __restrict__ dst, long n,
                                                    int bf, const float* __restrict__ minus) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT)
        dst[i] = minus ? sld1(src, i, bf) - sld1(minus, i, bf) : sld1(src, i, bf);
}


// ------------------------------------------------------------ clip_grad_norm_ + Adam over the flat blobs, two launches
// train.py:282-285: torch.nn.utils.clip_grad_norm_(model.parameters(), 3.0); optimizer.step() (torch.optim.Adam, no
// amsgrad, L2 weight decay 0 by default).  In PyTorch that is one norm kernel per tensor + stack + norm + a foreach
// multiply, then the foreach Adam over 248 views: ~300 launches and ~200 tiny buffer copies per step for 19 014 floats.
// Parameters, gradients and both moments are views of four flat blobs in the canonical layout here:
//  k_grad_sqsum  one element per thread, sum of squares of the masked gradient in double per workgroup (fixed-order
//                tree); the LAST workgroup to arrive (a ticket from one atomic counter; the partials were published with a
//                device-scope fence) adds the partials in index order -- the arrival order does not enter the result --
//                and stores the total norm and the clip coefficient min(max_norm / (norm + 1e-6), 1), exactly what
//                clip_grad_norm_ computes; it also resets the counter for the next step
//  k_adam_flat   one element per thread: gradient scaled in place as clip_grad_norm_ leaves it, Adam moments and
//                parameter updated where the mask is set (BatchNorm running statistics and the ERB bank carry no
//                gradient and must not move)
// (A first version did both phases in ONE workgroup of 1024 threads, 44 elements per thread: each of its 88 trips
// paid a full memory latency and the "fused" step was 0.4 ms SLOWER than PyTorch's 300 launches, same-box A/B.)
constexpr int ADAM_NT = 256;
__global__ __launch_bounds__(ADAM_NT) void k_grad_sqsum(const float* __restrict__ g, const float* __restrict__ mask, int n,
                                                       float max_norm, double* __restrict__ partial,
                                                       unsigned* __restrict__ counter, float* __restrict__ out_norm) {
    __shared__ double sh[ADAM_NT];
    __shared__ unsigned ticket;
    const int tid = threadIdx.x, i = blockIdx.x * ADAM_NT + tid;
    double x = 0.0;
    if (i < n && mask[i] != 0.f) x = (double)g[i];
    sh[tid] = x * x;
    __syncthreads();
    for (int o = ADAM_NT / 2; o > 0; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        partial[blockIdx.x] = sh[0];
        __threadfence();                                   // the partial is visible device-wide before the ticket is
        ticket = atomicAdd(counter, 1u);
    }
    __syncthreads();
    if (ticket != gridDim.x - 1) return;
    __threadfence();
    double s = 0.0;
    for (int b = tid; b < (int)gridDim.x; b += ADAM_NT) s += __builtin_nontemporal_load(partial + b);
    sh[tid] = s;
    __syncthreads();
    for (int o = ADAM_NT / 2; o > 0; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        const float norm = (float)sqrt(sh[0]);
        float coef = 1.f;
        if (max_norm > 0.f) {
            coef = max_norm / (norm + 1e-6f);
            coef = coef > 1.f ? 1.f : coef;                // (a NaN norm stays NaN, as torch.clamp leaves it)
        }
        out_norm[0] = norm;
        out_norm[1] = coef;
        *counter = 0u;
    }
}

__global__ __launch_bounds__(ADAM_NT) void k_adam_flat(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                      float* __restrict__ v, const float* __restrict__ mask, int n,
                                                      int clip, float beta2, float omb1, float omb2, float step_size,
                                                      float bc2_sqrt, float eps, float weight_decay,
                                                      const float* __restrict__ norm) {
    const int i = blockIdx.x * ADAM_NT + threadIdx.x;
    if (i >= n || mask[i] == 0.f) return;
    float gi = g[i], pi = p[i], mi = m[i], vi = v[i];
    if (clip) { gi *= norm[1]; g[i] = gi; }                     // clip_grad_norm_ scales the gradients in place
    if (weight_decay != 0.f) gi = fmaf(weight_decay, pi, gi);   // Adam's L2 form: grad += wd * param
    mi = mi + (gi - mi) * omb1;                                 // exp_avg.lerp_(grad, 1 - beta1)
    vi = fmaf(vi, beta2, omb2 * gi * gi);                       // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    pi = pi - step_size * (mi / denom);                         // param.addcdiv_(exp_avg, denom, value=-step_size)
    m[i] = mi; v[i] = vi; p[i] = pi;
}

int check() { return (int)hipGetLastError(); }

// One launch: the kernel named once, its arguments once.
template <class... P, class... A>
void launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, const A&... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
}

// Run-time value -> template argument (the integer twin of with_flags in kernels.hip): calls f with the
// std::integral_constant of the admitted value that equals v.  False when v is none of them: nothing was launched and
// the launcher refuses the call.
template <auto... Vs, class V, class F>
bool dispatch(V v, F&& f) {
    return ((v == Vs ? (f(std::integral_constant<decltype(Vs), Vs>{}), true) : false) || ...);
}
// ... and a pair of values -> one of the listed Case<A, B>s.  Pairs are ENUMERATED, never the cross-product of two
// dispatches: only the listed instantiations exist in the code object (no kernel stores bf16 gradients next to fp32
// activations, none recomputes x without a riding reduction).
template <auto A, auto B> struct Case { static constexpr auto a = A; static constexpr auto b = B; };
template <class... Cs, class VA, class VB, class F>
bool dispatch_case(VA a, VB b, F&& f) {
    return ((a == Cs::a && b == Cs::b ? (f(Cs{}), true) : false) || ...);
}
// storage format of one tensor where the kernel has a general form for everything but fp32 / bf16: that form's argument
inline int fmt_or(int bf, int other) { return bf == 0 || bf == 1 ? bf : other; }
// formats of a kernel's input and output tensor (.a, .b): fp32 / bf16 each, all four
template <class F>
bool with_io_fmt(int in_bf, int out_bf, F&& f) {
    return dispatch_case<Case<0, 0>, Case<1, 1>, Case<0, 1>, Case<1, 0>>(in_bf, out_bf, f);
}
// formats of a unit backward's saved activations and of the gradients handed between units (.a, .b): bf16 gradients go
// with bf16 activations only
template <class F>
bool with_grad_fmt(int bf, int gbf, F&& f) {
    return dispatch_case<Case<0, 0>, Case<1, 1>, Case<1, 0>>(bf, gbf ? 1 : 0, f);
}
// riding reduction of the unit in front (.a) and recomputation of x from that unit's y (.b), which needs the former
template <class F>
bool with_riding(bool nxt, bool xr, F&& f) {
    return dispatch_case<Case<false, false>, Case<true, false>, Case<true, true>>(nxt, xr, f);
}

// ---- in-launch finish: host side.  The trainer hands over its group-sum / counter buffers per call (thread local: one
// caller thread per trainer); `on` = fusion bit 10.
struct FinCtx { bool on = false; double* gpart = nullptr; unsigned* ctr = nullptr; };
thread_local FinCtx g_fin;
inline FinArgs fin_off() { FinArgs f{}; return f; }
inline FinArgs fin_stats(const StatFin* sf) {
    FinArgs f{};
    if (!g_fin.on || !sf || !g_fin.gpart) return f;
    f.kind = 1; f.C = sf->C; f.n = sf->n; f.gpart = g_fin.gpart; f.ctr = g_fin.ctr;
    f.o0 = sf->stats; f.o1 = sf->running_mean; f.o2 = sf->running_var; f.o3 = sf->shift; f.o4 = sf->stats_b;
    return f;
}
inline FinArgs fin_bwd(long n, int C, float* red, float* dgamma, float* dbeta, float* dslope) {
    FinArgs f{};
    if (!g_fin.on || !g_fin.gpart || n <= 0) return f;
    f.kind = 2; f.C = C; f.n = n; f.gpart = g_fin.gpart; f.ctr = g_fin.ctr;
    f.o0 = red; f.o1 = dgamma; f.o2 = dbeta; f.o3 = dslope;
    return f;
}
// the backward's means live in one of two slots behind the partial sums: a kernel that reads its unit's pair from one slot
// while its last workgroup writes the NEXT unit's pair uses the other
inline float* red_slot(double* dscratch, int slot) {
    return reinterpret_cast<float*>(dscratch + (long)MAX_PARTIALS * 3 * 16) + 32 * slot;
}
// have_parts of a backward launcher: > 0 partial sums wait in dscratch (finish kernel needed), 0 nothing yet, < 0 the
// producing kernel's last workgroup also ran the finish: the pair is in slot -have_parts - 1
inline int parts_slot(int have_parts) { return have_parts < 0 ? -have_parts - 1 : 0; }

}  // namespace

void set_fin_context(bool on, double* gpart, unsigned* ctr) { g_fin.on = on; g_fin.gpart = gpart; g_fin.ctr = ctr; }
// fusion bit 13: the pointwise forward convs through k_pw_fwd instead of the general k_conv_mfma<1, 1> (thread local, like g_fin)
static thread_local bool g_pw_form = true;
void set_pointwise_form(bool on) { g_pw_form = on; }
// fusion bit 15: the weight-gradient finishes of a backward pass recorded and run as a batch (see k_wgrad_finish_batch)
struct WDefer {
    bool on = false;
    float* pool = nullptr;
    size_t cap = 0, used = 0;         // floats
    int n = 0;
    WFin list[64];
};
static thread_local WDefer g_wdefer;
void set_wgrad_defer(bool on, float* pool, size_t cap_floats) {
    g_wdefer.on = on && pool; g_wdefer.pool = pool; g_wdefer.cap = cap_floats; g_wdefer.used = 0; g_wdefer.n = 0;
}
// a region of the pool for one unit's partial sums, or nullptr (deferral off, pool or list full: finish right away)
static float* wdefer_take(size_t nfloats) {
    nfloats = (nfloats + 63) & ~(size_t)63;
    if (!g_wdefer.on || g_wdefer.n >= 64 || g_wdefer.used + nfloats > g_wdefer.cap) return nullptr;
    float* p = g_wdefer.pool + g_wdefer.used;
    g_wdefer.used += nfloats;
    return p;
}
static void wdefer_conv(const ConvGeom& g, const float* partial, int nparts, float* dw, float* dbias) {
    const int ntap = g.nkt * g.nkf;
    g_wdefer.list[g_wdefer.n++] = WFin{partial, dw, dbias, nparts, ntap * 256 + 16, 0, ntap, g.nkf, g.Cout, g.Cin, g.w_co, g.w_ci, g.w_kt, g.w_kf};
}
static void wdefer_dw(const DwGeom& g, const double* partial, int nparts, float* dw, float* dbias) {
    const int ntap = g.nkt * g.nkf;
    g_wdefer.list[g_wdefer.n++] = WFin{partial, dw, dbias, nparts, (ntap + 1) * 16, 1, ntap, g.nkf, 16, 16, g.w_c, g.w_kt, g.w_kf, 0};
}
int flush_wgrad_finishes(hipStream_t s) {
    for (int i0 = 0; i0 < g_wdefer.n; i0 += WFIN_BATCH) {
        WFinBatch b{};
        b.n = g_wdefer.n - i0 < WFIN_BATCH ? g_wdefer.n - i0 : WFIN_BATCH;
        int kmax = 0;
        for (int i = 0; i < b.n; ++i) { b.e[i] = g_wdefer.list[i0 + i]; kmax = b.e[i].K > kmax ? b.e[i].K : kmax; }
        hipLaunchKernelGGL(k_wgrad_finish_batch, dim3((kmax + 63) / 64, b.n), dim3(1024), 0, s, b);
    }
    g_wdefer.n = 0;
    g_wdefer.used = 0;
    return check();
}
// fusion bit 14: the TCN's dilated depthwise forward in its column form (k_dw31_col)
static thread_local bool g_col_form = true;
void set_column_form(bool on) { g_col_form = on; }

// ====================================================================================== launchers
// grid of a streaming reduction: a stride that is a multiple of C (NT is), at most MAX_PARTIALS workgroups
static void launch_bn_bwd_reduce4(int grid, hipStream_t s, const float* da, const float* y, long total, int C,
                                  const float* stats, const float* gamma, const float* beta, const float* res, int act,
                                  const float* slope, double* partial, int bf, int ybf, const FinArgs& fa, int gbf = 0) {
    // FA: formats (.a; 0: all fp32, 5: bf16 activations, bf16 conv outputs) and activation (.b) as compile-time
    // constants, -1 where the kernel reads them at run time
    auto run = [&](auto FA, auto GF) {
        launch(k_bn_bwd_reduce<4, FA.a, FA.b, GF.value>, dim3(grid), dim3(NT), 0, s, da, y, total, C, stats, gamma, beta, res,
               act, slope, partial, bf, ybf, fa);
    };
    const int f = bf * 4 + ybf;
    if (gbf) {                                                       // bf16 gradient hand-offs (storage mode 5)
        auto run1 = [&](auto FA) { run(FA, std::integral_constant<int, 1>{}); };
        if (!dispatch_case<Case<5, ACT_PRELU>, Case<5, ACT_NONE>>(f, act, run1)) run1(Case<-1, -1>{});
    } else {
        auto run0 = [&](auto FA) { run(FA, std::integral_constant<int, 0>{}); };
        if (!dispatch_case<Case<0, ACT_PRELU>, Case<0, ACT_NONE>, Case<5, ACT_PRELU>, Case<5, ACT_NONE>>(f, act, run0) &&
            !dispatch_case<Case<0, -1>, Case<5, -1>>(f, -1, run0))
            run0(Case<-1, -1>{});
    }
}

static int red_grid(long units) {
    long g = (units + NT * 8 - 1) / (NT * 8);       // >= 8 elements per thread
    if (g < 1) g = 1;
    if (g > MAX_PARTIALS) g = MAX_PARTIALS;
    return (int)g;
}

// First pass of a unit's backward (C % 4 == 0): sum dz, sum dz xhat, the slope terms, then the means and dgamma / dbeta /
// dslope.  Either the kernel that produced da has done all of it (have_parts < 0, in-launch finish), or its partial sums
// wait in dscratch (have_parts > 0: the finish kernel), or the pass runs now -- with its finish in its own last
// workgroup when the context is on.  Returns the slot that holds the unit's means (red_slot).
static int bwd_first_pass(int have_parts, hipStream_t s, const float* da, const float* y, long n, int C, const float* stats,
                          const float* gamma, const float* beta, const float* res, int act, const float* slope,
                          double* dscratch, int bf, int ybf, float* dgamma, float* dbeta, float* dslope, int gbf = 0) {
    if (have_parts < 0) return parts_slot(have_parts);
    float* red = red_slot(dscratch, 0);
    if (have_parts > 0) {
        hipLaunchKernelGGL(k_bn_bwd_finish, dim3(1), dim3(1024), 0, s, dscratch, have_parts, n, C, red, dgamma, dbeta, dslope);
        return 0;
    }
    const int rgrid = red_grid(n * C / 4);
    const FinArgs fa = fin_bwd(n, C, red, dgamma, dbeta, dslope);
    launch_bn_bwd_reduce4(rgrid, s, da, y, n * C, C, stats, gamma, beta, res, act, slope, dscratch, bf, ybf, fa, gbf);
    if (!fa.kind)
        hipLaunchKernelGGL(k_bn_bwd_finish, dim3(1), dim3(1024), 0, s, dscratch, rgrid, n, C, red, dgamma, dbeta, dslope);
    return 0;
}
// the riding reduction's in-launch finish: that unit's means go into the slot this launch does NOT read
static FinArgs next_fin(bool nxt, const DwUnitNext* next, double* dscratch, int slot) {
    return nxt ? fin_bwd(next->n, 16, red_slot(dscratch, 1 - slot), next->dgamma, next->dbeta, next->dslope) : fin_off();
}
// ... and what the launcher reports for it (the have_parts of that unit's backward): the slot, or `grid` partial sums
static void set_next_parts(int* next_parts, bool nxt, const FinArgs& nfa, int slot, int grid) {
    if (nxt && next_parts) *next_parts = nfa.kind ? -1 - (1 - slot) : grid;
}
// the riding reduction's view of the unit in front: its y and BatchNorm / PReLU constants (nothing without one).  res,
// xround and yfmt differ between the kernels: their launchers fill them.
static NextRedArgs next_args(bool nxt, const DwUnitNext* next) {
    NextRedArgs nx{};
    if (nxt) nx = NextRedArgs{next->y, next->stats, next->gamma, next->beta, next->slope};
    return nx;
}
// the weight-gradient finish of a fused unit backward whose partial sums are `nparts` rows of `part`: recorded for
// the batch when they sit in a region of the deferral pool (fusion bit 15), launched now when in the caller's scratch
static void finish_wgrad(bool deferred, const ConvGeom& g, const float* part, int nparts, float* dw, float* dbias, hipStream_t s) {
    const int K = g.nkt * g.nkf * 256 + 16;
    if (deferred) wdefer_conv(g, part, nparts, dw, dbias);
    else launch(k_wgrad_mfma_finish, dim3((K + 63) / 64), dim3(1024), 0, s, g, part, nparts, dw, dbias);
}
static void finish_wgrad(bool deferred, const DwGeom& g, const double* part, int nparts, float* dw, float* dbias, hipStream_t s) {
    const int K = (g.nkt * g.nkf + 1) * 16;
    if (deferred) wdefer_dw(g, part, nparts, dw, dbias);
    else launch(k_dw_wgrad_finish2, dim3((K + 63) / 64), dim3(1024), 0, s, g, part, nparts, dw, dbias);
}

static bool mfma_ok(const ConvGeom& g) {
    return (g.Cin % 4) == 0 && (g.Cout % 4) == 0 && (g.CinT % 4) == 0 && (g.CoutT % 4) == 0 && (g.cin_off % 4) == 0 &&
           (g.cout_off % 4) == 0 && g.Fout >= 16 && g.sf <= 2 &&
           ((g.nkt == 1 && ((g.nkf == 1 && g.sf == 1) || (g.nkf == 5 && g.sf == 2))) ||
            (g.nkt == 3 && g.nkf == 3 && g.sf == 1));
}

// the window forms (see win_pos): a (1, nkf) conv with stride 2 between a tensor of exactly 16 channels and a narrow
// one whose nkf * C window fits the 16 columns of the MFMA
static bool win_fwd_ok(const ConvGeom& g) {
    return g.f_mode == 0 && g.nkt == 1 && g.t_off[0] == 0 && g.Tin == g.Tout && g.sf == 2 && g.Cin * g.nkf <= 16 &&
           g.CinT == g.Cin && g.cin_off == 0 && (g.Cout % 4) == 0 && (g.CoutT % 4) == 0 && (g.cout_off % 4) == 0 &&
           g.Cout <= 16 && g.Fout >= 16;
}
static bool win_wgrad_ok(const ConvGeom& g) {
    if (g.nkt != 1 || g.t_off[0] != 0 || g.Tin != g.Tout || g.sf != 2) return false;
    if (g.f_mode == 0)
        return g.Cin * g.nkf <= 16 && g.CinT == g.Cin && g.cin_off == 0 && g.Cout == 16 && g.CoutT == 16 && g.cout_off == 0;
    return g.Cout * g.nkf <= 16 && g.CoutT == g.Cout && g.cout_off == 0 && g.Cin == 16 && g.CinT == 16 && g.cin_off == 0;
}

int conv_fwd(const ConvGeom& g, const float* in, const float* w, const float* bias, float* out, hipStream_t s,
             double* stat_partial, int* stat_parts, const float* shift, const BnPre* pre, const DwUnitNext* next,
             int next_yfmt, const StatFin* sf) {
    if (shift && !g.out_bf) return (int)hipErrorInvalidValue;
    if (g.out2) return (int)hipErrorInvalidValue;      // (a second output copy: the 3-channel depthwise conv only)
    if (stat_parts) *stat_parts = 0;
    const BnPre nopre{};
    const NextRedArgs nonx{};
    // in-launch finish: of this unit's statistics (forward, sf) or of the riding reduction (backward, next->n > 0)
    const FinArgs fa = next ? fin_bwd(next->n, 16, red_slot(stat_partial, 0), next->dgamma, next->dbeta, next->dslope)
                            : fin_stats(sf);
    if (next) {
        // a backward launch whose output is the gradient input of the unit `next` (16 channels, PReLU, no residual):
        // that unit's BatchNorm reduction rides in the epilogue -- per-workgroup sums in stat_partial, their count in
        // *stat_parts (hand it to that unit's backward as have_parts)
        if (!stat_partial || !stat_parts || pre || shift || next->res || !next->slope || !mfma_ok(g) || g.in_bf != 0 ||
            g.Cout != 16 || g.CoutT != 16 || g.cout_off != 0 ||
            !((g.nkt == 3 && g.nkf == 3) || (g.nkt == 1 && g.nkf == 5)))
            return (int)hipErrorInvalidValue;
        const long ntiles = ((long)g.B * g.Tout * g.Fout + 15) / 16;
        long waves = (long)MAX_PARTIALS * 4;
        if (waves > ntiles) waves = ntiles;
        const long tpw = (ntiles + waves - 1) / waves;
        const int grid = (int)((ntiles + tpw * 4 - 1) / (tpw * 4));
        NextRedArgs nx = next_args(true, next);
        nx.yfmt = next_yfmt;
        if (next_yfmt < 0 || next_yfmt > 1) return (int)hipErrorInvalidValue;
        dispatch_case<Case<3, 3>, Case<1, 5>>(g.nkt, g.nkf, [&](auto K) {
            dispatch<0, 1>(next_yfmt, [&](auto YF) {
                launch(k_conv_mfma<K.a, K.b, 0, false, false, 1 + YF.value>, dim3(grid), dim3(NT), 0, s, g, in, w, bias, out, tpw,
                       stat_partial, shift, nopre, nx, fa);
            });
        });
        *stat_parts = fa.kind ? -1 : grid;           // (folded: that unit's means are in slot 0)
        return check();
    }
    if (pre && g.nkt == 3 && g.nkf == 3) {
        // the decoder's dense transposed 3x3 behind a deferred unit (depth_conv <- point_conv1): the LDS-tiled form
        if (g.t_off[0] != 0 || g.t_off[1] != -1 || g.t_off[2] != -2 || g.f_mode != 1 || g.sf != 1 || g.pf != 1 || g.Fin != 33 ||
            g.Fout != 33 || g.Cin != 16 || g.CinT != 16 || g.cin_off != 0 || g.Cout != 16 || g.CoutT != 16 || g.cout_off != 0 ||
            g.Tout != g.Tin + 2 || g.in_bf != (pre->exact ? 0 : pre->ybf) || g.in_bf > 1 || g.accumulate || pre->res || !stat_partial ||
            !stat_parts)
            return (int)hipErrorInvalidValue;
        const int tiles_t = (g.Tout + F33_TF - 1) / F33_TF;
        const long ntiles = (long)g.B * tiles_t;
        const int gridt = (int)(ntiles < MAX_PARTIALS ? ntiles : MAX_PARTIALS);
        dispatch<0, 1>(g.in_bf, [&](auto FI) {
            launch(k_dense33_fwd_pre<FI.value>, dim3(gridt), dim3(NT), 0, s, g, in, w, bias, out, stat_partial, shift, *pre, tiles_t, fa);
        });
        *stat_parts = fa.kind ? -gridt : gridt;
        return check();
    }
    if (pre && !(mfma_ok(g) && g.nkt == 1 && g.nkf == 1 && g.sf == 1 && g.Cin == 16 && g.CinT == 16 && g.cin_off == 0 &&
                 g.in_bf == pre->ybf))
        return (int)hipErrorInvalidValue;
    if (!pre && win_fwd_ok(g) && stat_parts && !g.accumulate && g.Cout == 16 && g.CoutT == 16 && g.cout_off == 0) {
        // forward of a unit (a BatchNorm follows): the reference-ordered fmaf chain (see k_conv_win_fma)
        const long units = (long)g.B * g.Tout * g.Fout * 4;
        double* sp = stat_partial;
        const int g16 = grid_for(units, sp ? MAX_PARTIALS : 16384);
        const StrideIter it = stride_iter((long)g16 * NT / 4, g.Fout, g.Tout);
        const FinArgs fw = sp ? fa : fin_off();
        dispatch<0, 1, 2>(fmt_or(g.in_bf, 2), [&](auto FI) {
            launch(k_conv_win_fma<FI.value>, dim3(g16), dim3(NT), 0, s, g, in, w, bias, out, sp, it, shift, fw);
        });
        if (sp) *stat_parts = fw.kind ? -g16 : g16;
        return check();
    }
    const bool win = win_fwd_ok(g);
    if (win || mfma_ok(g)) {
        const long ntiles = ((long)g.B * g.Tout * g.Fout + 15) / 16;
        long waves = 256L * 4 * 4;                       // 4 workgroups of 4 waves per CU
        if (waves > ntiles) waves = ntiles;
        const long tpw = (ntiles + waves - 1) / waves;
        const int grid = (int)((ntiles + tpw * 4 - 1) / (tpw * 4));
        double* sp = (stat_partial && stat_parts && grid <= MAX_PARTIALS && g.cout_off == 0 && g.Cout == g.CoutT &&
                      !g.accumulate) ? stat_partial : nullptr;
        const FinArgs fm = sp ? fa : fin_off();
        // the dedicated pointwise form (see k_pw_fwd): a pure 1x1 conv over flat positions, whole output tensor, 0 / bf16 formats
        const bool pw = !win && g.nkt == 1 && g.nkf == 1 && g.t_off[0] == 0 && g.Tin == g.Tout && g.Fin == g.Fout && g.sf == 1 &&
                        g.pf == 0 && g.f_mode == 0 && !g.accumulate && g.cout_off == 0 && g.Cout == g.CoutT && g.in_bf <= 1 && g.out_bf <= 1 &&
                        (long)g.B * g.Tout * g.Fout * 16 < (1L << 31) && (!pre || (!pre->exact && pre->bf == g.in_bf)) &&
                        g_pw_form;
        // ... and the two 16 -> 16 (1,5) stride-2 layers (see k_c15_fwd)
        const bool c15 = !win && !pre && g_pw_form && g.nkt == 1 && g.nkf == 5 && g.t_off[0] == 0 && g.Tin == g.Tout && g.sf == 2 &&
                         g.pf == 2 && g.w_kf == 1 && g.Cin == 16 && g.CinT == 16 && g.cin_off == 0 && g.Cout == 16 && g.CoutT == 16 &&
                         g.cout_off == 0 && !g.accumulate && g.in_bf <= 1 && g.out_bf <= 1 &&
                         ((g.f_mode == 0 && g.Fin == 65 && g.Fout == 33) || (g.f_mode == 1 && g.Fin == 33 && g.Fout == 65)) &&
                         (long)g.B * g.Tout * 65 * 16 < (1L << 31);
        if (c15) {
            const long npos = (long)g.B * g.Tout * g.Fout;
            with_io_fmt(g.in_bf, g.out_bf, [&](auto IO) {
                dispatch<false, true>(g.f_mode != 0, [&](auto TR) {
                    launch(k_c15_fwd<IO.a, IO.b, TR.value>, dim3(grid), dim3(NT), 0, s, npos, g.w_co, g.w_ci, in, w, bias, out,
                           tpw, sp, shift, fm);
                });
            });
        } else if (pw) {
            const long npos = (long)g.B * g.Tout * g.Fout;
            // PR (.a): behind a deferred unit; RS (.b): that unit has a residual input
            dispatch_case<Case<true, true>, Case<true, false>, Case<false, false>>(pre != nullptr, pre && pre->res, [&](auto PR) {
                with_io_fmt(g.in_bf, g.out_bf, [&](auto IO) {
                    launch(k_pw_fwd<IO.a, IO.b, PR.a, PR.b>, dim3(grid), dim3(NT), 0, s, npos, g.Cin, g.CinT, g.cin_off,
                           g.Cout, g.w_co, g.w_ci, in, w, bias, out, tpw, sp, shift, pre ? *pre : nopre, fm);
                });
            });
        } else {
            // the general kernel: its (1, 1) form behind a deferred unit or as the window form, else by the layer's taps
            dispatch<0, 1, 2>(fmt_or(g.in_bf, 2), [&](auto FI) {
                if (pre)
                    launch(k_conv_mfma<1, 1, FI.value, false, true>, dim3(grid), dim3(NT), 0, s, g, in, w, bias, out, tpw, sp, shift,
                           *pre, nonx, fm);
                else if (win)
                    launch(k_conv_mfma<1, 1, FI.value, true>, dim3(grid), dim3(NT), 0, s, g, in, w, bias, out, tpw, sp, shift, nopre,
                           nonx, fm);
                else
                    dispatch_case<Case<3, 3>, Case<1, 5>, Case<1, 1>>(g.nkt, g.nkf, [&](auto K) {
                        launch(k_conv_mfma<K.a, K.b, FI.value>, dim3(grid), dim3(NT), 0, s, g, in, w, bias, out, tpw, sp, shift,
                               nopre, nonx, fm);
                    });
            });
        }
        if (sp) *stat_parts = fm.kind ? -grid : grid;
        return check();
    }
    const int grid = grid_for((long)g.B * g.Tout * g.Fout);
    if ((long)g.B * g.Tout * g.Fout >= (1L << 31)) return (int)hipErrorInvalidValue;      // (k_conv divides in 32 bits)
    // de_convs.4 forward / en_convs.0's data gradient: the LDS-staged, parity-sorted form (see k_thin_tr_fm)
    if (g.nkt == 1 && g.nkf == 5 && g.f_mode == 1 && g.sf == 2 && g.pf == 2 && g.Fin == 65 && g.Fout == 129 && g.Cin == 16 &&
        g.CinT == 16 && g.cin_off == 0 && (g.Cout == 2 || g.Cout == 3) && g.CoutT == g.Cout && g.cout_off == 0 && !g.accumulate &&
        g.w_kf == 1 && g.Tin == g.Tout && g.t_off[0] == 0 && g.in_bf <= 1 && g.out_bf <= 1) {
        const long nrows = (long)g.B * g.Tout;
        const int gt = grid_for((nrows + 3) / 4 * NT, 2048);
        dispatch<2, 3>(g.Cout, [&](auto CO) {
            with_io_fmt(g.in_bf, g.out_bf, [&](auto IO) {
                launch(k_thin_tr_fm<CO.value, IO.a, IO.b>, dim3(gt), dim3(NT), 0, s, nrows, g.w_co, g.w_ci, in, w, bias, shift, out);
            });
        });
        return check();
    }
    // the direct form: the channel counts (.a in, .b out) of this model's thin layers
    if (!dispatch_case<Case<3, 16>, Case<16, 3>, Case<16, 16>, Case<8, 16>, Case<16, 8>, Case<16, 2>, Case<2, 16>>(
            g.Cin, g.Cout, [&](auto C) {
                launch(k_conv<C.a, C.b>, dim3(grid), dim3(NT), 0, s, g, in, w, bias, out, shift);
            }))
        return (int)hipErrorInvalidValue;
    return check();
}

int conv_wgrad(const ConvGeom& g, const float* in, const float* dout, float* dw, float* dbias, float* scratch,
               hipStream_t s) {
    if (win_wgrad_ok(g)) {
        const bool wide_in = g.f_mode != 0;
        const long ngroups = ((long)g.B * g.Tin * (wide_in ? g.Fin : g.Fout) + 3) / 4;
        long waves = (long)MAX_PARTIALS * WG_WAVES;
        if (waves > ngroups) waves = ngroups;
        long gpw = (ngroups + waves - 1) / waves;
        gpw = (gpw + 3) & ~3L;                           // whole 16-position tiles per wave
        const int grid = (int)((ngroups + gpw * WG_WAVES - 1) / (gpw * WG_WAVES));
        dispatch<0, 1, 2>(fmt_or(g.in_bf, 2), [&](auto FI) {
            dispatch<false, true>(wide_in, [&](auto WIDE) {
                launch(k_wgrad_win<FI.value, WIDE.value>, dim3(grid), dim3(WG_WAVES * 64), 0, s, g, in, dout, scratch, gpw);
            });
        });
        hipLaunchKernelGGL(k_wgrad_win_finish, dim3(5), dim3(1024), 0, s, g, scratch, grid, dw, dbias, wide_in ? 1 : 0);
        return check();
    }
    if (g.Fout >= 4 && g.sf <= 2 && ((g.nkt == 1 && (g.nkf == 1 || g.nkf == 5)) || (g.nkt == 3 && g.nkf == 3))) {
        const long ngroups = ((long)g.B * g.Tout * g.Fout + 3) / 4;
        long waves = (long)MAX_PARTIALS * WG_WAVES;
        if (waves > ngroups) waves = ngroups;
        const long gpw = (ngroups + waves - 1) / waves;
        const int grid = (int)((ngroups + gpw * WG_WAVES - 1) / (gpw * WG_WAVES));
        const int K = g.nkt * g.nkf * 256 + 16;
        // 16-byte operand loads through wave-private LDS tiles when the channel counts allow them (all MFMA layers of
        // this model); the 4-byte form otherwise
        const bool wide = mfma_ok(g);     // channel counts / offsets in multiples of four: 16-byte operand loads
        dispatch_case<Case<3, 3>, Case<1, 5>, Case<1, 1>>(g.nkt, g.nkf, [&](auto K) {
            dispatch<0, 1, 2>(fmt_or(g.in_bf, 2), [&](auto FI) {
                if (wide) launch(k_conv_wgrad_lds<K.a, K.b, FI.value>, dim3(grid), dim3(WG_WAVES * 64), 0, s, g, in, dout, scratch, gpw);
                else launch(k_conv_wgrad_mfma<K.a, K.b, FI.value>, dim3(grid), dim3(WG_WAVES * 64), 0, s, g, in, dout, scratch, gpw);
            });
        });
        hipLaunchKernelGGL(k_wgrad_mfma_finish, dim3((K + 63) / 64), dim3(1024), 0, s, g, scratch, grid, dw, dbias);
        return check();
    }
    (void)in; (void)dout; (void)dw; (void)dbias; (void)scratch;
    return (int)hipErrorInvalidValue;     // no such convolution in this model
}

int dw_fwd(const DwGeom& g, const float* in, const float* w, const float* bias, float* out, hipStream_t s,
           double* stat_partial, int* stat_parts, const float* shift, const BnPre* pre, const DwUnitNext* next,
           int next_yfmt, const StatFin* sf) {
    if (shift && (!g.out_bf || g.C != 16)) return (int)hipErrorInvalidValue;
    if (g.out2 && (g.out_bf || g.accumulate || g.C != 3)) return (int)hipErrorInvalidValue;
    if (stat_parts) *stat_parts = 0;
    const BnPre nopre{};
    const NextRedArgs nonx{};
    const FinArgs fa = next ? fin_bwd(next->n, 16, red_slot(stat_partial, 0), next->dgamma, next->dbeta, next->dslope)
                            : fin_stats(sf);            // see conv_fwd
    if (next) {      // see conv_fwd
        if (!stat_partial || !stat_parts || pre || shift || next->res || !next->slope || g.C != 16 || g.nkt != 3 ||
            g.nkf != 3 || g.in_bf != 0 || g.Tin != g.Tout)
            return (int)hipErrorInvalidValue;
        const int g16 = grid_for((long)g.B * g.Tout * g.F * 4, MAX_PARTIALS);
        const StrideIter it = stride_iter((long)g16 * NT / 4, g.F, g.Tout);
        if (next_yfmt < 0 || next_yfmt > 1) return (int)hipErrorInvalidValue;
        NextRedArgs nx = next_args(true, next);
        nx.yfmt = next_yfmt;
        dispatch<0, 1>(next_yfmt, [&](auto YF) {
            launch(k_dw16<3, 3, 0, false, 1 + YF.value>, dim3(g16), dim3(NT), 0, s, g, in, w, bias, out, stat_partial, it, shift,
                   nopre, nx, fa);
        });
        *stat_parts = fa.kind ? -1 : g16;
        return check();
    }
    if (pre && g.C == 16 && g.nkt == 3 && g.nkf == 3) {
        // depthwise 3x3 behind a deferred unit (encoder depth_conv <- point_conv1): the LDS-tiled form
        if (g.F != 33 || g.t_off[0] != -2 || g.t_off[1] != -1 || g.t_off[2] != 0 || g.f_off[0] != -1 || g.f_off[1] != 0 ||
            g.f_off[2] != 1 || g.Tin != g.Tout || g.in_bf != (pre->exact ? 0 : pre->ybf) || g.in_bf > 1 || g.accumulate || pre->res ||
            !stat_partial || !stat_parts)
            return (int)hipErrorInvalidValue;
        const int tiles_t = (g.Tout + F33_TF - 1) / F33_TF;
        const long ntiles = (long)g.B * tiles_t;
        const int gridt = (int)(ntiles < MAX_PARTIALS ? ntiles : MAX_PARTIALS);
        dispatch<0, 1>(g.in_bf, [&](auto FI) {
            launch(k_dw33_fwd_pre<FI.value>, dim3(gridt), dim3(NT), 0, s, g, in, w, bias, out, stat_partial, shift, *pre, tiles_t, fa);
        });
        *stat_parts = fa.kind ? -gridt : gridt;
        return check();
    }
    if (pre && !(g.C == 16 && g.nkt == 3 && g.nkf == 1 && g.t_off[2] == 0 && g.f_off[0] == 0 && g.in_bf == pre->ybf &&
                 g.in_bf <= 1 && !g.accumulate && !pre->res))
        return (int)hipErrorInvalidValue;
    const int grid = grid_for((long)g.B * g.Tout * g.F);
    if (g.C == 16) {
        double* sp = (stat_partial && stat_parts && !g.accumulate) ? stat_partial : nullptr;
        const FinArgs fd = sp ? fa : fin_off();
        const int g16 = grid_for((long)g.B * g.Tout * g.F * 4, sp ? MAX_PARTIALS : 16384);
        if (g.Tin != g.Tout) return (int)hipErrorInvalidValue;
        const StrideIter it = stride_iter((long)g16 * NT / 4, g.F, g.Tout);
        // the column form (see k_dw31_col): the TCN's dilated (3,1) conv behind its deferred unit, fusion bit 14
        const int dil = -g.t_off[1];
        if (pre && g_col_form && sp && dil >= 1 && g.t_off[0] == -2 * dil && g.w_kf == 1 && !pre->exact && pre->bf == g.in_bf &&
            g.out_bf <= 1 && !g.out2 && (long)g.B * g.Tout * g.F * 16 < (1L << 31)) {
            const int cj = g.in_bf ? DcChunk<1>::J : DcChunk<0>::J;
            const long items = (long)g.B * dil * (((g.Tout + dil - 1) / dil + cj - 1) / cj) * g.F * 4;
            const int gc = grid_for(items, MAX_PARTIALS);
            with_io_fmt(g.in_bf, g.out_bf, [&](auto IO) {
                launch(k_dw31_col<IO.a, IO.b>, dim3(gc), dim3(NT), 0, s, g.B, g.Tout, g.F, dil, g.w_c, g.w_kt, in, w, bias, out, sp,
                       shift, *pre, fd);
            });
            *stat_parts = fd.kind ? -gc : gc;
            return check();
        }
        // (3, 1) behind a deferred unit, the (3, 3) / (3, 1) forms with the input format at compile time (-1: read at
        // run time), or the form for any taps
        const bool taps3 = g.nkt == 3 && (g.nkf == 3 || g.nkf == 1);
        if (pre)
            dispatch<0, 1>(g.in_bf, [&](auto FI) {
                launch(k_dw16<3, 1, FI.value, true>, dim3(g16), dim3(NT), 0, s, g, in, w, bias, out, sp, it, shift, *pre, nonx, fd);
            });
        else if (taps3)
            dispatch<3, 1>(g.nkf, [&](auto KF) {
                dispatch<0, 1, -1>(fmt_or(g.in_bf, -1), [&](auto FI) {
                    launch(k_dw16<3, KF.value, FI.value>, dim3(g16), dim3(NT), 0, s, g, in, w, bias, out, sp, it, shift, nopre, nonx, fd);
                });
            });
        else
            launch(k_dw16<0, 0>, dim3(g16), dim3(NT), 0, s, g, in, w, bias, out, sp, it, shift, nopre, nonx, fd);
        if (sp) *stat_parts = fd.kind ? -g16 : g16;
        return check();
    }
    else if (g.C == 3) hipLaunchKernelGGL((k_dw<3>), dim3(grid), dim3(NT), 0, s, g, in, w, bias, out);
    else return (int)hipErrorInvalidValue;
    return check();
}

int dw_wgrad(const DwGeom& g, const float* in, const float* dout, float* dw, float* dbias, float* scratch,
             hipStream_t s) {
    if (g.C == 16 && ((g.nkt == 3 && g.nkf == 3) || (g.nkt == 3 && g.nkf == 1))) {
        double* part = reinterpret_cast<double*>(scratch);      // <= MAX_PARTIALS * 160 doubles
        const int grid = red_grid((long)g.B * g.Tout * g.F * 4);
        const int K = (g.nkt * g.nkf + 1) * 16;
        if (g.Tin != g.Tout) return (int)hipErrorInvalidValue;
        const StrideIter it = stride_iter((long)grid * NT / 4, g.F, g.Tout);
        dispatch<3, 1>(g.nkf, [&](auto KF) {
            dispatch<0, 1, -1>(fmt_or(g.in_bf, -1), [&](auto FI) {
                launch(k_dw_wgrad_stream<3, KF.value, FI.value>, dim3(grid), dim3(NT), 0, s, g, in, dout, part, it);
            });
        });
        hipLaunchKernelGGL(k_dw_wgrad_finish2, dim3((K + 63) / 64), dim3(1024), 0, s, g, part, grid, dw, dbias);
        return check();
    }
    if (g.C == 3 && g.nkt == 1 && g.nkf == 3 && g.f_off[0] == -1 && g.f_off[2] == 1 && g.w_c == 3 && g.w_kf == 1) {
        double* part = reinterpret_cast<double*>(scratch);
        const long rows = (long)g.B * g.Tout;
        const int grid = red_grid(rows * g.F);
        hipLaunchKernelGGL(k_sfe_wgrad, dim3(grid), dim3(NT), 0, s, in, dout, rows, g.F, part, g.in_bf);
        hipLaunchKernelGGL(k_sfe_wgrad_finish, dim3(1), dim3(1024), 0, s, part, grid, dw);
        return check();
    }
    return (int)hipErrorInvalidValue;     // no such depthwise convolution in this model
}

int bn_stats(const float* y, long n, int C, float* stats, float* running_mean, float* running_var, double* scratch,
             hipStream_t s, int have_parts, int bf, float* shifted, float* stats_b) {
    const long total = n * C;
    if (have_parts < 0) return 0;    // the producing conv's last workgroup finished the statistics (in-launch finish)
    if (have_parts > 0) {     // the producing conv already left its per-workgroup sums in scratch
        hipLaunchKernelGGL(k_bn_stats_finish, dim3(1), dim3(1024), 0, s, scratch, have_parts, n, C, stats, running_mean,
                           running_var, shifted, stats_b);
        return check();
    }
    const StatFin sf{n, C, stats, running_mean, running_var, shifted, stats_b};
    const FinArgs fa = fin_stats(&sf);
    const int vec = C % 4 == 0 ? 4 : 1;      // elements per thread and load
    const int grid = red_grid(total / vec);
    dispatch<4, 1>(vec, [&](auto V) { launch(k_bn_stats<V.value>, dim3(grid), dim3(NT), 0, s, y, total, C, scratch, bf, fa); });
    if (!fa.kind)
        hipLaunchKernelGGL(k_bn_stats_finish, dim3(1), dim3(1024), 0, s, scratch, grid, n, C, stats, running_mean,
                           running_var, shifted, stats_b);
    return check();
}

int bn_act(const float* y, long n, int C, const float* stats, const float* gamma, const float* beta,
           const float* res, int act, const float* slope, float* a, hipStream_t s, int bf, int ybf, float* a2,
           int a2_bf, float* y2, int y2_bf, const float* post) {
    const long total = n * C;
    if (post && (a2 || y2)) return (int)hipErrorInvalidValue;      // (the exact chain adds its sums in passes of their own)
    if (C % 4 == 0)
        hipLaunchKernelGGL((k_bn_act<4>), dim3(grid_for(total / 4, 8192)), dim3(NT), 0, s, y, total, C, stats, gamma,
                           beta, res, act, slope, a, bf, ybf, a2, a2_bf, y2, y2_bf, post);
    else
        hipLaunchKernelGGL((k_bn_act<1>), dim3(grid_for(total, 8192)), dim3(NT), 0, s, y, total, C, stats, gamma, beta,
                           res, act, slope, a, bf, ybf, a2, a2_bf, y2, y2_bf, post);
    return check();
}

int bn_act_bwd(const float* da, const float* y, long n, int C, const float* stats, const float* gamma,
               const float* beta, const float* res, int act, const float* slope, float* dy, float* dres,
               int dres_acc, float* dgamma, float* dbeta, float* dslope, double* scratch, hipStream_t s, int bf,
               int ybf, int have_parts, int gbf) {
    const long total = n * C;
    if (gbf && (C % 4 != 0 || !bf)) return (int)hipErrorInvalidValue;      // (bf16 gradients: the 16-bit modes' wide units)
    if (C % 4 == 0) {
        const int slot = bwd_first_pass(have_parts, s, da, y, n, C, stats, gamma, beta, res, act, slope, scratch, bf, ybf,
                                        dgamma, dbeta, dslope, gbf);
        // the apply pass keeps per-thread channel constants: its stride must be a multiple of C as well
        hipLaunchKernelGGL((k_bn_bwd_apply<4>), dim3(grid_for(total / 4, 8192)), dim3(NT), 0, s, da, y, total, C, stats,
                           gamma, beta, res, act, slope, red_slot(scratch, slot), dy, dres, dres_acc, bf, ybf, gbf);
    } else {
        float* red = red_slot(scratch, 0);
        const int grid = red_grid(total);
        const FinArgs fa = fin_bwd(n, C, red, dgamma, dbeta, dslope);
        hipLaunchKernelGGL((k_bn_bwd_reduce<1>), dim3(grid), dim3(NT), 0, s, da, y, total, C, stats, gamma, beta, res,
                           act, slope, scratch, bf, ybf, fa);
        if (!fa.kind)
            hipLaunchKernelGGL(k_bn_bwd_finish, dim3(1), dim3(1024), 0, s, scratch, grid, n, C, red, dgamma, dbeta, dslope);
        hipLaunchKernelGGL((k_bn_bwd_apply<1>), dim3(grid_for(total, 8192)), dim3(NT), 0, s, da, y, total, C, stats,
                           gamma, beta, res, act, slope, red, dy, dres, dres_acc, bf, ybf, 0);
    }
    return check();
}

constexpr int DC_BWD_GRID = 512;  // workgroups of k_dwunit31_col (see the register counts in its launcher)
constexpr int NEXT_GRID = 768;    // workgroups of k_unit1x1_bwd<.., NEXT>: 126-138 VGPRs = 3 per CU, all resident
int dwunit_bwd(const DwGeom& g, const float* x, const float* y, const float* da, const float* stats,
               const float* gamma, const float* beta, const float* slope, const float* w, float* dx, float* dw,
               float* dbias, float* dgamma, float* dbeta, float* dslope, double* dscratch, float* fscratch,
               hipStream_t s, int bf, int ybf, const DwUnitNext* next, int* next_parts, int have_parts, int gbf) {
    if (next_parts) *next_parts = 0;
    if (g.C != 16 || g.nkt != 3 || g.nkf != 1 || g.t_off[2] != 0 || g.f_off[0] != 0 || g.t_off[0] != 2 * g.t_off[1] ||
        g.Tin != g.Tout || !slope || !dx || bf > 1 || ybf > 1 || bf != ybf || (gbf && !bf))
        return (int)hipErrorInvalidValue;
    const long n = (long)g.B * g.Tout * g.F, total = n * 16;
    const int slot = bwd_first_pass(have_parts, s, da, y, n, 16, stats, gamma, beta, nullptr, ACT_PRELU, slope, dscratch, bf, ybf,
                                    dgamma, dbeta, dslope, gbf);
    float* red = red_slot(dscratch, slot);
    // 164 VGPRs: three workgroups per CU -- a grid of 3 x 256 keeps every workgroup resident (with 1024 the last 256
    // would run alone at a third of the occupancy)
    const int grid = red_grid(total / 4) > 768 ? 768 : red_grid(total / 4);
    const StrideIter it = stride_iter((long)grid * NT / 4, g.F, g.Tout);
    const bool nxt = next && next->slope;
    const bool xr = nxt && next->recompute_x;
    if (!x && !xr) return (int)hipErrorInvalidValue;          // (before a region of the deferral pool is taken)
    float* const dpool = wdefer_take((size_t)MAX_PARTIALS * 64 * 2);     // (both forms' grids fit)
    if (dpool) fscratch = dpool;
    double* wpart = reinterpret_cast<double*>(fscratch);      // [grid][64]
    BnBwdArgs bn{stats, gamma, beta, slope, red, ACT_PRELU};
    NextRedArgs nx = next_args(nxt, next);
    if (nxt) nx.xround = next->recompute_x == 2;
    const FinArgs nfa = next_fin(nxt, next, dscratch, slot);
    int nparts = grid;
    if (g_col_form && nxt && total < (1L << 31)) {       // the column form (see k_dwunit31_col), fusion bit 14
        const int dil = -g.t_off[1];
        const int cj = (bf && gbf) ? DcBwdChunk<1, 1>::J : DcBwdChunk<0, 0>::J;
        const long items = (long)g.B * dil * (((g.Tout + dil - 1) / dil + cj - 1) / cj) * g.F * 4;
        const int gc = (int)((items + NT - 1) / NT < DC_BWD_GRID ? (items + NT - 1) / NT : DC_BWD_GRID);
        with_grad_fmt(bf, gbf, [&](auto FMT) {
            dispatch<false, true>(xr, [&](auto XR) {
                launch(k_dwunit31_col<FMT.a, FMT.b, XR.value>, dim3(gc), dim3(NT), 0, s, g.B, g.Tout, g.F, dil, g.w_c, g.w_kt, x, y,
                       da, bn, w, dx, wpart, nx, dscratch, nfa);
            });
        });
        nparts = gc;
    } else {
        with_grad_fmt(bf, gbf, [&](auto FMT) {
            with_riding(nxt, xr, [&](auto RIDE) {
                launch(k_dwunit31_bwd<FMT.a, FMT.a, RIDE.a, RIDE.b, FMT.b>, dim3(grid), dim3(NT), 0, s, g, x, y, da, bn, w, dx,
                       wpart, nx, dscratch, it, nfa);
            });
        });
    }
    finish_wgrad(dpool != nullptr, g, wpart, nparts, dw, dbias, s);
    set_next_parts(next_parts, nxt, nfa, slot, nparts);
    return check();
}

int dwunit33_bwd(const DwGeom& g, const float* x, const float* y, const float* da, const float* stats,
                 const float* gamma, const float* beta, const float* slope, const float* w, float* dx, float* dw,
                 float* dbias, float* dgamma, float* dbeta, float* dslope, double* dscratch, float* fscratch,
                 hipStream_t s, int bf, int ybf, const DwUnitNext* next, int* next_parts, int have_parts, int gbf) {
    if (next_parts) *next_parts = 0;
    if (gbf && !bf) return (int)hipErrorInvalidValue;
    if (g.C != 16 || g.F != 33 || g.nkt != 3 || g.nkf != 3 || g.t_off[0] != -2 || g.t_off[1] != -1 || g.t_off[2] != 0 ||
        g.f_off[0] != -1 || g.f_off[1] != 0 || g.f_off[2] != 1 || g.Tin != g.Tout || !slope || !dx || bf > 1 || ybf > 1 ||
        bf != ybf)
        return (int)hipErrorInvalidValue;
    const long n = (long)g.B * g.Tout * g.F;
    const int slot = bwd_first_pass(have_parts, s, da, y, n, 16, stats, gamma, beta, nullptr, ACT_PRELU, slope, dscratch, bf, ybf,
                                    dgamma, dbeta, dslope, gbf);
    float* red = red_slot(dscratch, slot);
    const int tiles_t = (g.Tout + D33_TF - 1) / D33_TF;
    const long ntiles = (long)g.B * tiles_t;
    // 64 KB of LDS: two workgroups per CU, 512 resident -- whole rounds of them
    const int grid = (int)(ntiles < 512 ? ntiles : 512);
    const bool nxt = next && next->slope && !next->res;
    const bool xr = nxt && next->recompute_x;
    if (!x && !xr) return (int)hipErrorInvalidValue;          // (before a region of the deferral pool is taken)
    float* const dpool = wdefer_take((size_t)grid * 160 * 2);
    if (dpool) fscratch = dpool;
    double* wpart = reinterpret_cast<double*>(fscratch);      // [grid][160]
    BnBwdArgs bn{stats, gamma, beta, slope, red, ACT_PRELU};
    NextRedArgs nx = next_args(nxt, next);
    if (nxt) { nx.xround = next->recompute_x == 2; nx.yfmt = ybf; }
    const FinArgs nfa = next_fin(nxt, next, dscratch, slot);
    with_grad_fmt(bf, gbf, [&](auto FMT) {
        with_riding(nxt, xr, [&](auto RIDE) {
            launch(k_dwunit33_bwd<FMT.a, FMT.a, RIDE.a, RIDE.b, FMT.b>, dim3(grid), dim3(NT), 0, s, g, x, y, da, bn, w, dx, wpart,
                   nx, dscratch, tiles_t, nfa);
        });
    });
    finish_wgrad(dpool != nullptr, g, wpart, grid, dw, dbias, s);
    set_next_parts(next_parts, nxt, nfa, slot, grid);
    return check();
}

int dense33_bwd(const ConvGeom& g, const float* x, const float* y, const float* da, const float* stats,
                const float* gamma, const float* beta, const float* slope, const float* w, float* dx, float* dw,
                float* dbias, float* dgamma, float* dbeta, float* dslope, double* dscratch, float* fscratch,
                hipStream_t s, int bf, int ybf, const DwUnitNext* next, int* next_parts, int have_parts, int gbf) {
    if (next_parts) *next_parts = 0;
    if (gbf && !bf) return (int)hipErrorInvalidValue;
    // the decoder's ConvTranspose2d(16,16,(3,3),padding (0,1)) in gather form: taps t, t-1, t-2, transposed in frequency
    if (g.nkt != 3 || g.nkf != 3 || g.t_off[0] != 0 || g.t_off[1] != -1 || g.t_off[2] != -2 || g.f_mode != 1 || g.sf != 1 ||
        g.pf != 1 || g.Fin != 33 || g.Fout != 33 || g.Cin != 16 || g.CinT != 16 || g.cin_off != 0 || g.Cout != 16 ||
        g.CoutT != 16 || g.cout_off != 0 || g.Tout != g.Tin + 2 || !slope || !dx || bf > 1 || ybf > 1 || bf != ybf)
        return (int)hipErrorInvalidValue;
    const long n = (long)g.B * g.Tout * g.Fout;
    const int slot = bwd_first_pass(have_parts, s, da, y, n, 16, stats, gamma, beta, nullptr, ACT_PRELU, slope, dscratch, bf, ybf,
                                    dgamma, dbeta, dslope, gbf);
    float* red = red_slot(dscratch, slot);
    const int tiles_t = (g.Tout + D9_TF - 1) / D9_TF;
    const long ntiles = (long)g.B * tiles_t;
    const int grid = (int)(ntiles < 512 ? ntiles : 512);           // 72 KB of LDS: two workgroups per CU, all resident
    BnBwdArgs bn{stats, gamma, beta, slope, red, ACT_PRELU};
    const bool nxt = next && next->slope && !next->res;
    const bool xr = nxt && next->recompute_x;
    if (!x && !xr) return (int)hipErrorInvalidValue;
    NextRedArgs nx = next_args(nxt, next);
    if (nxt) { nx.xround = next->recompute_x == 2; nx.yfmt = ybf; }
    const FinArgs nfa = next_fin(nxt, next, dscratch, slot);
    float* const dpool = wdefer_take((size_t)grid * (9 * 256 + 16));
    if (dpool) fscratch = dpool;
    // (the attribute belongs to the current device's copy of the kernel: set on every launch -- a host-side table lookup --
    // rather than remembered per process, which would miss a second device)
    hipError_t e = hipSuccess;
    with_grad_fmt(bf, gbf, [&](auto FMT) {
        with_riding(nxt, xr, [&](auto RIDE) {
            const auto kernel = k_dense33_bwd<FMT.a, FMT.a, RIDE.a, RIDE.b, FMT.b>;
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    D9_LDS_FLOATS * 4);
            if (e == hipSuccess)
                launch(kernel, dim3(grid), dim3(NT), D9_LDS_FLOATS * 4, s, g, x, y, da, bn, w, dx, fscratch, nx, dscratch, tiles_t, nfa);
        });
    });
    if (e != hipSuccess) return (int)e;
    finish_wgrad(dpool != nullptr, g, fscratch, grid, dw, dbias, s);
    set_next_parts(next_parts, nxt, nfa, slot, grid);
    return check();
}

int conv15_bwd(const ConvGeom& g, const float* x, const float* y, const float* da, const float* stats,
               const float* gamma, const float* beta, const float* slope, const float* w, float* dx, int dx_acc,
               float* dw, float* dbias, float* dgamma, float* dbeta, float* dslope, double* dscratch, float* fscratch,
               hipStream_t s, int bf, int ybf, const DwUnitNext* next, int* next_parts, int have_parts, int gbf) {
    if (next_parts) *next_parts = 0;
    if (gbf && !bf) return (int)hipErrorInvalidValue;
    const bool dyw = g.f_mode == 1;
    if (g.nkt != 1 || g.nkf != 5 || g.t_off[0] != 0 || g.sf != 2 || g.pf != 2 || g.Cin != 16 || g.CinT != 16 || g.cin_off != 0 ||
        g.Cout != 16 || g.CoutT != 16 || g.cout_off != 0 || g.Tin != g.Tout || g.Fin != (dyw ? 33 : 65) || g.Fout != (dyw ? 65 : 33) ||
        !slope || !dx || !x || bf > 1 || ybf > 1 || bf != ybf || (next && dyw))
        return (int)hipErrorInvalidValue;
    const long n = (long)g.B * g.Tout * g.Fout;
    const int slot = bwd_first_pass(have_parts, s, da, y, n, 16, stats, gamma, beta, nullptr, ACT_PRELU, slope, dscratch, bf, ybf,
                                    dgamma, dbeta, dslope, gbf);
    float* red = red_slot(dscratch, slot);
    const int tiles_t = (g.Tout + C15_TF - 1) / C15_TF;
    const long ntiles = (long)g.B * tiles_t;
    const int grid = (int)(ntiles < 512 ? ntiles : 512);           // 61 KB of LDS: two workgroups per CU, all resident
    BnBwdArgs bn{stats, gamma, beta, slope, red, ACT_PRELU};
    const bool nxt = next && next->slope && !next->res;
    NextRedArgs nx = next_args(nxt, next);
    if (nxt) nx.yfmt = ybf;
    const FinArgs nfa = next_fin(nxt, next, dscratch, slot);
    float* const dpool = wdefer_take((size_t)grid * (5 * 256 + 16));
    if (dpool) fscratch = dpool;
    // the wide-output direction (.a), or the narrow one with or without a riding reduction (.b; refused above for the
    // wide one): the kernel's NEXT is 1 + the format of that unit's y
    dispatch_case<Case<true, false>, Case<false, true>, Case<false, false>>(dyw, nxt, [&](auto FORM) {
        with_grad_fmt(bf, gbf, [&](auto FMT) {
            launch(k_conv15_bwd<FORM.a, FMT.a, FMT.a, FORM.b ? 1 + FMT.a : 0, FMT.b>, dim3(grid), dim3(NT), 0, s, g, x, y, da, bn, w,
                   dx, dx_acc, fscratch, nx, dscratch, tiles_t, nfa);
        });
    });
    finish_wgrad(dpool != nullptr, g, fscratch, grid, dw, dbias, s);
    set_next_parts(next_parts, nxt, nfa, slot, grid);
    return check();
}

int unit1x1_bwd(const ConvGeom& g, const float* x, const float* y, const float* da, const float* res,
                const float* stats, const float* gamma, const float* beta, int act, const float* slope,
                const float* w, float* dx, int dx_acc, float* dres, int dres_acc, float* dw, float* dbias,
                float* dgamma, float* dbeta, float* dslope, double* dscratch, float* fscratch, hipStream_t s, int bf,
                int ybf, int have_parts, const DwUnitNext* next, int* next_parts, int gbf) {
    if (next_parts) *next_parts = 0;
    const long n = (long)g.B * g.Tout * g.Fout;
    if (g.nkt != 1 || g.nkf != 1 || g.sf != 1 || g.pf != 0 || g.Cout != g.CoutT || g.cout_off != 0 || (g.Cout % 4) ||
        (g.Cin % 4) || (g.CinT % 4) || (g.cin_off % 4) || (gbf && !(bf == 1 && ybf == 1)) ||
        act == ACT_TANH ||                    // (the pointwise units are PReLU or linear: the kernel's derivative is one select)
        n * 16 >= (1L << 31))                 // (32-bit element offsets)
        return (int)hipErrorInvalidValue;
    const int slot = bwd_first_pass(have_parts, s, da, y, n, g.Cout, stats, gamma, beta, res, act, slope, dscratch, bf, ybf,
                                    dgamma, dbeta, dslope, gbf);
    float* red = red_slot(dscratch, slot);
    const long ntiles = (n + 15) / 16;
    // the unit in front takes this dx as its gradient input: its reduction rides along (its partial sums replace this
    // unit's, which the finish kernel above has consumed, in dscratch)
    const bool nxt = next && next->slope && dx && g.Cin == 16 && g.CinT == 16 && g.cin_off == 0 && bf == ybf;
    // (the recomputing form needs 120 VGPRs: four workgroups per CU, 1024 resident)
    const bool xr = nxt && next->recompute_x;
    long waves = (long)(nxt && !xr ? NEXT_GRID : MAX_PARTIALS) * (NT / 64);
    if (waves > ntiles) waves = ntiles;
    const long tpw = (ntiles + waves - 1) / waves;
    const int grid = (int)((ntiles + tpw * (NT / 64) - 1) / (tpw * (NT / 64)));
    BnBwdArgs bn{stats, gamma, beta, slope, red, act};
    if (!x && !xr) return (int)hipErrorInvalidValue;
    NextRedArgs nx = next_args(nxt, next);
    if (nxt) { nx.res = next->res; nx.xround = next->recompute_x == 2; }
    const FinArgs nfa = next_fin(nxt, next, dscratch, slot);
    float* const dpool = wdefer_take((size_t)grid * (256 + 16));      // (fusion bit 15: the finish is recorded, not launched)
    if (dpool) fscratch = dpool;
    // x / res and y in one format, fp32 or bf16
    if (bf != ybf || !with_grad_fmt(bf, gbf, [&](auto FMT) {
            with_riding(nxt, xr, [&](auto RIDE) {
                launch(k_unit1x1_bwd<FMT.a, FMT.a, RIDE.a, RIDE.b, FMT.b>, dim3(grid), dim3(NT), 0, s, g, x, y, da, res, bn, w, dx,
                       dx_acc, dres, dres_acc, fscratch, tpw, nx, dscratch, nfa);
            });
        }))
        return (int)hipErrorInvalidValue;
    finish_wgrad(dpool != nullptr, g, fscratch, grid, dw, dbias, s);
    set_next_parts(next_parts, nxt, nfa, slot, grid);
    return check();
}

// Layouts of a (B, 257, T, 2) spectrogram given by its strides in floats.  The two special forms make 8-byte (re, im)
// accesses: even strides and an 8-byte aligned base, which is what a complex tensor viewed as real has; anything else
// takes the generic form.
static bool pair_ok(const float* p, long sb, long sf, long st) {
    return ((sb | sf | st) & 1) == 0 && (reinterpret_cast<uintptr_t>(p) & 7) == 0;
}
static long ab(long v) { return v < 0 ? -v : v; }
// dense frame-major: LDS-staged frames
static bool frame_major(const float* p, long sb, long sf, long st, int T) {
    return sf == 2 && st == 514 && sb == (long)T * 514 && pair_ok(p, sb, sf, st);
}
// frame axis fastest (torch.stft's layout): tiles of TT frames, lanes along t
static bool time_major(const float* p, long sb, long sf, long st) { return ab(st) < ab(sf) && pair_ok(p, sb, sf, st); }

int feat_fwd(const float* spec, long sb, long sf, long st, int B, int T, const float* erb_w, float* eb,
             hipStream_t s, int bf, float* eb2, int eb2_bf) {
    if (frame_major(spec, sb, sf, st, T))
        hipLaunchKernelGGL(k_feat_fm, dim3(grid_for(((long)B * T + FM_NF - 1) / FM_NF * NT, 2048)), dim3(NT), 0, s, spec, (long)B * T,
                           erb_w, eb, bf, eb2, eb2_bf);
    else if (time_major(spec, sb, sf, st))
        hipLaunchKernelGGL(k_feat_t, dim3(B * ((T + TT - 1) / TT)), dim3(NT), 0, s, spec, sb, sf, st, B, T, erb_w, eb, bf,
                           eb2, eb2_bf);
    else
        hipLaunchKernelGGL(k_feat, dim3(grid_for((long)B * T * 129)), dim3(NT), 0, s, spec, sb, sf, st, B, T, erb_w, eb, bf,
                           eb2, eb2_bf);
    return check();
}
int bs_mask_fwd(const float* m, const float* spec, long sb, long sf, long st, int B, int T, const float* ierb_w,
                float* out, long ob, long of, long ot, hipStream_t s, int bf) {
    if (frame_major(spec, sb, sf, st, T) && frame_major(out, ob, of, ot, T))
        hipLaunchKernelGGL(k_bs_mask_fm, dim3(grid_for(((long)B * T + FM_NF - 1) / FM_NF * NT, 2048)), dim3(NT), 0, s, m, spec,
                           (long)B * T, ierb_w, out, bf);
    else if (time_major(spec, sb, sf, st) && time_major(out, ob, of, ot))
        hipLaunchKernelGGL(k_bs_mask_t, dim3(B * ((T + TT - 1) / TT)), dim3(NT), 0, s, m, spec, sb, sf, st, B, T, ierb_w,
                           out, ob, of, ot, bf);
    else
        hipLaunchKernelGGL(k_bs_mask, dim3(grid_for((long)B * T * 257)), dim3(NT), 0, s, m, spec, sb, sf, st, B, T, ierb_w,
                           out, ob, of, ot, bf);
    return check();
}
int bs_mask_bwd(const float* dout, long ob, long of, long ot, const float* spec, long sb, long sf, long st, int B,
                int T, const float* ierb_w, float* dm, hipStream_t s) {
    if (frame_major(spec, sb, sf, st, T) && frame_major(dout, ob, of, ot, T))
        hipLaunchKernelGGL(k_bs_mask_bwd_fm, dim3(grid_for(((long)B * T + FM_NF - 1) / FM_NF * NT, 2048)), dim3(NT), 0, s, dout, spec,
                           (long)B * T, ierb_w, dm);
    else if (time_major(spec, sb, sf, st) && time_major(dout, ob, of, ot))
        hipLaunchKernelGGL(k_bs_mask_bwd_t, dim3(B * ((T + TT - 1) / TT)), dim3(NT), 0, s, dout, ob, of, ot, spec, sb, sf,
                           st, B, T, ierb_w, dm);
    else
        hipLaunchKernelGGL(k_bs_mask_bwd, dim3(grid_for((long)B * T * 129)), dim3(NT), 0, s, dout, ob, of, ot, spec, sb, sf,
                           st, B, T, ierb_w, dm);
    return check();
}

static BnLoad bn_load(const TraBn* tb) {
    BnLoad b{};
    if (tb && tb->stats) b = BnLoad{tb->stats, tb->gamma, tb->beta, tb->ybf};
    return b;
}
int tra_fwd(const float* v, int B, int Tt, const float* dw_w, const float* dw_b, const float* pw_w,
            const float* pw_b, float* e, float* y, float* g, hipStream_t s, int bf, const TraBn* tb) {
    const long rows = (long)B * Tt;
    hipLaunchKernelGGL(k_tra_energy, dim3(grid_for(rows * 8)), dim3(NT), 0, s, v, rows, e, bf, bn_load(tb));
    hipLaunchKernelGGL(k_tra_gate, dim3(grid_for(rows * 8)), dim3(NT), 0, s, e, B, Tt, dw_w, dw_b, pw_w, pw_b, y, g);
    return check();
}
int gate_shuffle_fwd(const float* v, const float* g, const float* x, int B, int T, int Tt, float* out, hipStream_t s,
                     int bf, float* out2, int out2_bf, const float* skip, const TraBn* tb) {
    if (skip && out2) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gate_shuffle, dim3(grid_for((long)B * T * 33 * 2)), dim3(NT), 0, s, v, g, x, B, T, Tt, out, bf,
                       out2, out2_bf, skip, bn_load(tb));
    return check();
}
int tra_gate_shuffle_bwd(const float* dout, const float* v, const float* g, const float* e, const float* y, int B,
                         int T, int Tt, const float* dw_w, const float* pw_w, float* dv, float* dx, float* d_dw_w,
                         float* d_dw_b, float* d_pw_w, float* d_pw_b, float* tmp, float* scratch, hipStream_t s,
                         int bf, int dx_acc, const TraBn* tb, int gbf) {
    const long rows = (long)B * Tt;
    float* dzg = tmp;
    float* dy = tmp + rows * 8;
    hipLaunchKernelGGL(k_tra_dgate, dim3(grid_for(rows * 64, 8192)), dim3(NT), 0, s, dout, v, g, B, T, Tt, dzg, bf, bn_load(tb), gbf);
    hipLaunchKernelGGL(k_tra_dy, dim3(grid_for(rows * 8)), dim3(NT), 0, s, dzg, rows, pw_w, dy);
    hipLaunchKernelGGL(k_gate_shuffle_bwd, dim3(grid_for(rows * 33 * 2)), dim3(NT), 0, s, dout, g, dy, v, dw_w, B, T, Tt, dv,
                       dx, bf, dx_acc, bn_load(tb), gbf);
    const int parts = (int)(rows < MAX_PARTIALS ? rows : MAX_PARTIALS);
    hipLaunchKernelGGL(k_tra_pgrad, dim3(parts), dim3(1024), 0, s, dzg, y, dy, e, B, Tt, scratch);
    // the four gradients are contiguous in the blob in exactly the partials' order (d_dw_w is the first)
    (void)d_dw_b; (void)d_pw_w; (void)d_pw_b;
    hipLaunchKernelGGL(k_reduce_partials_f, dim3(2), dim3(1024), 0, s, scratch, parts, 104, d_dw_w);
    return check();
}

int hybrid_loss_spec(const float* pred, long pb, long pf, long pt, const float* tru, long tb, long tf, long tt, int B,
                     int T, float* grad, long gb, long gf, long gt, double* partial, int* parts, hipStream_t s) {
    const int grid = red_grid((long)B * 257 * T);
    if ((long)B * 257 * T >= (1L << 31)) return (int)hipErrorInvalidValue;       // (k_hloss_spec divides in 32 bits)
    dispatch<false, true>(ab(pt) > ab(pf), [&](auto FM) {
        launch(k_hloss_spec<FM.value>, dim3(grid), dim3(NT), 0, s, pred, pb, pf, pt, tru, tb, tf, tt, B, T, grad, gb, gf, gt, partial);
    });
    *parts = grid;
    return check();
}
int sisnr_terms(float* yp, const float* yt, int B, long Lw, const double* spec_partial, int spec_parts, long N,
                const float* win, double* dwork, float* coef, float* loss, int want_grad, hipStream_t s) {
    if (B > 1024) return (int)hipErrorInvalidValue;
    const int chunks = SISNR_CHUNKS;
    double* part = dwork;                      // B * chunks * 3
    double* vals = dwork + (long)B * chunks * 3;
    hipLaunchKernelGGL(k_sisnr_sums, dim3(chunks, B), dim3(NT), 0, s, yp, yt, Lw, part);
    hipLaunchKernelGGL(k_sisnr_coef, dim3(1), dim3(1024), 0, s, part, chunks, B, N, spec_partial, spec_parts, coef, vals,
                       loss);
    if (want_grad)
        hipLaunchKernelGGL(k_sisnr_gwave, dim3(grid_for((long)B * Lw, 8192)), dim3(NT), 0, s, yp, yt, Lw, (long)B * Lw,
                           coef, win);
    return check();
}

int add_saved(const float* a, const float* b, float* out, long n, hipStream_t s, int bf) {
    if (n % 4) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_add_saved, dim3(grid_for(n / 4, 8192)), dim3(NT), 0, s, a, b, out, n / 4, bf);
    return check();
}
int saved_to_f32(const float* src, float* dst, long n, hipStream_t s, int bf, const float* minus) {
    hipLaunchKernelGGL(k_saved_to_f32, dim3(grid_for(n, 8192)), dim3(NT), 0, s, src, dst, n, bf, minus);
    return check();
}

int clip_adam(float* p, float* g, float* m, float* v, const float* mask, int n, float max_norm, float beta1, float beta2,
              float omb1, float omb2, float step_size, float bc2_sqrt, float eps, float weight_decay, float* out_norm,
              double* partial, unsigned* counter, hipStream_t s) {
    (void)beta1;
    const int grid = (n + ADAM_NT - 1) / ADAM_NT;
    hipLaunchKernelGGL(k_grad_sqsum, dim3(grid), dim3(ADAM_NT), 0, s, g, mask, n, max_norm, partial, counter, out_norm);
    hipLaunchKernelGGL(k_adam_flat, dim3(grid), dim3(ADAM_NT), 0, s, p, g, m, v, mask, n, max_norm > 0.f ? 1 : 0, beta2,
                       omb1, omb2, step_size, bc2_sqrt, eps, weight_decay, out_norm);
    return check();
}
int add(const float* a, const float* b, float* out, long n, hipStream_t s) {
    hipLaunchKernelGGL(k_add, dim3(grid_for(n)), dim3(NT), 0, s, a, b, out, n);
    return check();
}

}  // namespace gtt
