// kernels.hip -- gfx950 (MI355X / CDNA4) kernels of the GTCRN-Micro hot path.
//
// Design (DESIGN.md has the long form):
//   * one workgroup (11 waves) owns one utterance / stream and walks it in time
//     chunks of TC = 16 frames; causal history lives in LDS rings, so nothing is
//     recomputed and chunked == offline == streaming by construction.
//   * every 16-channel activation is a "slot-space" tile: 16 consecutive
//     (frame, bin) positions x 16 slots = the C/D fragment of
//     v_mfma_f32_16x16x4_f32 (weights are the A operand, activations the B
//     operand), so chains of 1x1 convs run register to register and only the
//     spatial taps go through LDS.  fp32 MFMA is exact fp32 (k-ordered fma).
//   * elementwise work (bias via the C operand, PReLU, depthwise taps, gates)
//     rides on the VALU next to the MFMA pipe.
// Reference semantics are cited per function (paths relative to the reference repo).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "fft256.h"
#include "kernels.h"
#include "layout.h"

using namespace gtl;
using namespace gtfft;

namespace gtk {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// ----------------------------------------------------------------------------- helpers
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
// parameter segment -> LDS, 16 bytes per lane (segment offsets and sizes are multiples of four floats, layout.h)
__device__ __forceinline__ void copy_params(float* dst, const float* src, int n, int tid, int nthr) {
    for (int i = 4 * tid; i < n; i += 4 * nthr) st4(dst + i, ld4(src + i));
}
__device__ __forceinline__ f32x4 splat(float v) { f32x4 r = {v, v, v, v}; return r; }
// Parameter segments -> LDS by LDS-DMA (global_load_lds_dwordx4): one instruction moves 1 KB (64 lanes x 16 bytes) from
// per-lane global addresses to a wave-uniform LDS base, holds no registers while in flight and is counted in vmcnt, so a
// later `s_waitcnt vmcnt(N)` + barrier publishes it.  (Inline asm: with the builtin the compiler would put vmcnt(0) in
// front of the next LDS read; it does not know these instructions, so every wait IT inserts for a register load that
// is issued later also drains them -- in-order return -- and a group must be issued behind the consumption of the
// register loads it is meant to overlap with.)
__device__ __forceinline__ void lds_dma_1k(const float* gsrc_lane, const float* lds_piece) {
    const unsigned lds_dst = (unsigned)(size_t)(__attribute__((address_space(3))) const void*)lds_piece;
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc_lane), "s"(lds_dst)
                 : "memory");
}
struct DmaSeg {
    int src, dst, n;      // float offsets of the segment in the global parameter buffer / in LDS, floats (a multiple of 4)
};
// A GROUP of segments, cut into 1 KB pieces that are dealt round-robin to the NWAVES waves: every wave issues EXACTLY
// PER_WAVE instructions (the counted waits need one number for all waves), a wave whose turn runs past the last piece
// repeats piece 0 -- the same bytes to the same place.  The last piece of a segment is partial: its tail lanes sit out.
template <int NSEG, int PER_WAVE, int NWAVES>
__device__ __forceinline__ void lds_dma_group(const DmaSeg (&seg)[NSEG], const float* gbase, float* lbase, int wave, int lane) {
    int total = 0;
#pragma unroll
    for (int k = 0; k < NSEG; ++k) total += (seg[k].n + 255) >> 8;
#pragma unroll
    for (int j = 0; j < PER_WAVE; ++j) {
        int pi = wave + j * NWAVES;
        if (pi >= total) pi = 0;
        int src = 0, dst = 0, n = 0;
#pragma unroll
        for (int k = NSEG - 1; k >= 0; --k) {            // the segment piece pi falls into (pieces are numbered segment by segment)
            int first = 0;
#pragma unroll
            for (int q = 0; q < k; ++q) first += (seg[q].n + 255) >> 8;
            if (pi >= first && n == 0) { src = seg[k].src + (pi - first) * 256; dst = seg[k].dst + (pi - first) * 256; n = seg[k].n - (pi - first) * 256; }
        }
        if (4 * lane < n) lds_dma_1k(gbase + src + 4 * lane, lbase + dst);
    }
}

// Workgroup barrier for LDS hand-offs only.  __syncthreads() carries a workgroup-scope release
// fence, which on gfx950 drains vmcnt: every barrier would then wait for all global loads and
// stores in flight (prefetches, skip-tensor stores).  Waves of a workgroup exchange data only
// through LDS here, so waiting for this wave's LDS operations (lgkmcnt) is sufficient.
// (LDS data that only the lanes of ONE wave exchange: wave_lds_sync, fft256.h)
__device__ __forceinline__ void wg_barrier() {
#ifdef GT_EXP_NOBARRIER      // timing experiment only (results are wrong): what the barrier skew costs
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#else
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#endif
}
// ... that also publishes this wave's LDS-DMA writes (global_load_lds: counted in vmcnt)
// KEEP = vector-memory operations issued AFTER the DMA that may stay in flight (vmcnt retires in issue order)
template <int KEEP = 0>
__device__ __forceinline__ void wg_barrier_vm() {
#ifdef GT_EXP_NOBARRIER
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(KEEP) : "memory");
#else
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(KEEP) : "memory");
#endif
}

// position-major LDS image: one record of 16 floats per position, slot group g at +16g bytes, records RS floats apart.
// Unswizzled on purpose: tap addresses are then "own address + compile-time constant", which keeps address arithmetic
// off the VALU.  RS = 16 (dense 64-byte records) costs a 2-way bank conflict on every tile-wide ds_read_b128 (its
// lane groups are {0-3,12-15,20-27}, ...: eight lanes of one slot group land on four 16-byte bank slots) and a 4-way
// one on ds_write_b128; RS = 24 (96-byte pitch) is conflict-free for reads at ANY base record (slot = (6 R + g) mod
// 16: the eight g-even lanes take the even slots, the eight g-odd lanes the odd ones) and 2-way for writes:
// 4.2 vs 7.4 and 14 vs 27 cycles per wave-instruction (tools/ubench_lds.hip).  The images of the offline encoder use
// RS = 24; kernels whose LDS budget has no room for the 50 % larger images keep RS = 16.
constexpr int RS_WIDE = 24;
template <int RS = 16>
__device__ __forceinline__ int pl(int pos, int g) { return pos * RS + 4 * g; }
__device__ __forceinline__ int pls(int pos, int slot) { return pos * 16 + slot; }

// float offset of lane (n, g)'s A-operand fragment inside a 16x16 slot matrix: columns 4g..4g+3 of row n; the packer
// stores rows 4..7 and 12..15 with their halves exchanged so that the ds_read_b128 is bank-conflict free (pack.cpp)
__device__ __forceinline__ int arow(int n, int g) { return n * 16 + 4 * (g ^ ((n >> 1) & 2)); }

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// PReLU with one shared slope a (nn.PReLU(), num_parameters = 1): x + (a-1) * min(x, 0); am1 = a - 1.
__device__ __forceinline__ f32x4 prelu4(f32x4 v, float am1) {
    f32x4 r;
    r[0] = fmaf(am1, fminf(v[0], 0.f), v[0]);
    r[1] = fmaf(am1, fminf(v[1], 0.f), v[1]);
    r[2] = fmaf(am1, fminf(v[2], 0.f), v[2]);
    r[3] = fmaf(am1, fminf(v[3], 0.f), v[3]);
    return r;
}
// sum over the 16 lanes of a DPP row (= the 16 positions of a tile, same slot group), result in
// every lane; fixed order, so results are reproducible run to run.
template <int CTRL>
__device__ __forceinline__ float dpp_ror(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float row_sum16(float v) {
    v += dpp_ror<0x128>(v);  // row_ror:8
    v += dpp_ror<0x124>(v);  // row_ror:4
    v += dpp_ror<0x122>(v);  // row_ror:2
    v += dpp_ror<0x121>(v);  // row_ror:1
    return v;
}
__device__ __forceinline__ float fast_tanh(float x) {
    // tanh(x) = 1 - 2 / (exp(2x) + 1); v_exp_f32 / v_rcp_f32 are ~1 ulp, far inside the 1e-4 budget
    const float t = __expf(2.0f * x);
    return 1.0f - 2.0f * __frcp_rn(t + 1.0f);
}

// ---- the int8-weight / fp16-activation variant (template flag Q; BASELINE configs[4]) -------------------------
// Every 16x16 slot-matrix product is ONE v_mfma_f32_16x16x16_f16 (fp16 operands, fp32 accumulate): its B operand
// holds k = 4g..4g+3 of column n and its D fragment rows 4g..4g+3 of column n, so -- exactly like the fp32 16x16x4
// form -- a layer's output fragment, converted to fp16, IS the next layer's B operand.  Weights arrive as
// int8-dequantised values (the host packer quantises the BatchNorm-folded weights per output channel, pack.cpp)
// and are exactly representable after the fp16 conversion up to 2^-11; activations are rounded to fp16 (RNE) where a
// layer produces them (rq), everything between two roundings is fp32.
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ h16x4 to_h4(const f32x4 v) {
    h16x4 r;
    r[0] = (_Float16)v[0]; r[1] = (_Float16)v[1]; r[2] = (_Float16)v[2]; r[3] = (_Float16)v[3];
    return r;
}
__device__ __forceinline__ f32x4 mfma_h(h16x4 a, h16x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0);
}
// rq / rq1: the contract's rounding of an activation, fp32 -> fp16 (RNE) -> fp32.  The fp32 value goes through an empty
// asm first: a multiply-add feeding the conversion is otherwise fused into v_fma_mixlo_f16, which rounds the exact
// sum ONCE to fp16 -- not the contract's fp32 sum rounded to fp16 (they differ where the fp32 sum is an fp16 tie: one
// element in ~10^4; tests/test_gpu_quant_stages.py holds the output stage to equality).
__device__ __forceinline__ float as_fp32_value(float v) {
    asm("" : "+v"(v));
    return v;
}
template <bool Q>
__device__ __forceinline__ float rq1(float v) {
    if constexpr (Q) return (float)(_Float16)as_fp32_value(v);
    else return v;
}
// The PReLU argument of prelu4q: the slope itself in the Q variant, slope - 1 otherwise (prelu4).
template <bool Q>
__device__ __forceinline__ float slope_arg(float slope) {
    if constexpr (Q) return slope;
    else return slope - 1.0f;
}
// Q: max(x, 0) + a * min(x, 0) -- a * x rounded once for x < 0, as the contract's checker forms it.  prelu4's
// x + (a - 1) * min(x, 0) rounds a - 1 first: a relative error of 2^-25 / a in the negative branch, harmless in fp32
// but enough, for a trained slope of a few 1e-3, to move one negative value in a hundred to the next fp16 number.
template <bool Q>
__device__ __forceinline__ f32x4 prelu4q(f32x4 v, float a) {
    if constexpr (Q) {
        f32x4 r;
        r[0] = fmaf(a, fminf(v[0], 0.f), fmaxf(v[0], 0.f));
        r[1] = fmaf(a, fminf(v[1], 0.f), fmaxf(v[1], 0.f));
        r[2] = fmaf(a, fminf(v[2], 0.f), fmaxf(v[2], 0.f));
        r[3] = fmaf(a, fminf(v[3], 0.f), fmaxf(v[3], 0.f));
        return r;
    } else {
        return prelu4(v, a);
    }
}
template <bool Q>
__device__ __forceinline__ f32x4 rq(const f32x4 v) {
    if constexpr (Q) {
        const f32x4 w = {as_fp32_value(v[0]), as_fp32_value(v[1]), as_fp32_value(v[2]), as_fp32_value(v[3])};
        const h16x4 h = to_h4(w);
        f32x4 r = {(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
        return r;
    } else {
        return v;
    }
}
// acc += M * b for one tile (M's fragment A, activations b)
template <bool Q>
__device__ __forceinline__ f32x4 mm1(const f32x4 A, const f32x4 b, f32x4 acc) {
    if constexpr (Q) {
        return mfma_h(to_h4(A), to_h4(b), acc);
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = mfma(A[s], b[s], acc);
        return acc;
    }
}
// acc[i] += M * x[i] for the wave's tiles: 4 k-steps, tiles interleaved so the dependent
// accumulator chains (40-cycle latency vs 32-cycle issue) overlap.
template <int N, bool Q = false>
__device__ __forceinline__ void mm16(const f32x4 A, const f32x4 (&x)[N], f32x4 (&acc)[N]) {
    if constexpr (Q) {
        const h16x4 ah = to_h4(A);
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] = mfma_h(ah, to_h4(x[i]), acc[i]);
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int i = 0; i < N; ++i) acc[i] = mfma(A[s], x[i][s], acc[i]);
    }
}

// ---- the dense 3x3 on the 16-bit matrix pipe ("split" form) --------------------------------
// fp32 MFMA (v_mfma_f32_16x16x4_f32) runs at the fp32 VALU rate and blocks the VALU while it does.  The decoder's
// dense transposed 3x3 (a 16 x 144 by 144 x 16 product per tile, 72 % of its matrix instructions) therefore runs on
// v_mfma_f32_16x16x32_bf16 instead, WITHOUT giving up fp32 accuracy: both operands are split exactly into three
// bf16 planes (x = hi + mid + lo: 3 x 8 significant bits are fp32's 24; every residual is exact in fp32) and the
// six partial products of weight >= 2^-16 are accumulated in fp32 (hi.hi, hi.mid, mid.hi, mid.mid, hi.lo, lo.hi; the
// dropped ones are <= 2^-24 relative).  30 instructions of 16 cycles that co-execute with the VALU replace 36 of 32
// cycles that do not; against float64 the result is as accurate as the fp32 chain (tools/ubench_split_bf16.hip:
// max 5.7e-7 vs 7.1e-7 of the output scale, 2.05x faster).  The weights are split by the host packer (layout.h
// D_DN16); h is split once where point_conv1 produces it and lives in LDS as three 32-byte planes per position --
// the same 96 bytes as the padded fp32 record it replaces.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
#ifdef GT_F32_DENSE
constexpr bool kSplitDense = false;     // A/B reference: the round-2 fp32-MFMA dense 3x3 (GT_EXP_FLAGS=-DGT_F32_DENSE
#else                                   // python tools/ab_bench.py; profiles/r03_ab_split_dense.txt)
constexpr bool kSplitDense = true;
#endif
#ifdef GT_F32_DENSE
constexpr bool kSplitDe3 = false;       // (part of the round-2 matrix path)
#else
constexpr bool kSplitDe3 = true;
#endif
struct Split3 {
    bf16x4 h, m, l;
};
__device__ __forceinline__ Split3 split3(const f32x4 v) {
    Split3 s;
    const f32x2 v01 = {v[0], v[1]}, v23 = {v[2], v[3]};
    const bf16x2 h01 = __builtin_convertvector(v01, bf16x2), h23 = __builtin_convertvector(v23, bf16x2);
    const f32x2 r01 = {v[0] - (float)h01[0], v[1] - (float)h01[1]}, r23 = {v[2] - (float)h23[0], v[3] - (float)h23[1]};
    const bf16x2 m01 = __builtin_convertvector(r01, bf16x2), m23 = __builtin_convertvector(r23, bf16x2);
    const f32x2 q01 = {r01[0] - (float)m01[0], r01[1] - (float)m01[1]}, q23 = {r23[0] - (float)m23[0], r23[1] - (float)m23[1]};
    const bf16x2 l01 = __builtin_convertvector(q01, bf16x2), l23 = __builtin_convertvector(q23, bf16x2);
    s.h[0] = h01[0]; s.h[1] = h01[1]; s.h[2] = h23[0]; s.h[3] = h23[1];
    s.m[0] = m01[0]; s.m[1] = m01[1]; s.m[2] = m23[0]; s.m[3] = m23[1];
    s.l[0] = l01[0]; s.l[1] = l01[1]; s.l[2] = l23[0]; s.l[3] = l23[1];
    return s;
}
// the inverse, exact: mid + lo has at most 16 significant bits, hi + (mid + lo) is the fp32 value that was split
__device__ __forceinline__ f32x4 join3(const bf16x4 h, const bf16x4 m, const bf16x4 l) {
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (float)h[e] + ((float)m[e] + (float)l[e]);
    return r;
}
// split record at float offset `rec` of an image with 24-float (96-byte) records: plane p at +8p floats, the lane's
// four slots 4g..4g+3 at +2g floats inside the plane
__device__ __forceinline__ void st_split(float* img, int rec, int g, const f32x4 v) {
    const Split3 s = split3(v);
    *reinterpret_cast<bf16x4*>(img + rec + 2 * g) = s.h;
    *reinterpret_cast<bf16x4*>(img + rec + 8 + 2 * g) = s.m;
    *reinterpret_cast<bf16x4*>(img + rec + 16 + 2 * g) = s.l;
}
__device__ __forceinline__ f32x4 ld_split(const float* img, int rec, int g) {
    return join3(*reinterpret_cast<const bf16x4*>(img + rec + 2 * g), *reinterpret_cast<const bf16x4*>(img + rec + 8 + 2 * g),
                 *reinterpret_cast<const bf16x4*>(img + rec + 16 + 2 * g));
}
__device__ __forceinline__ f32x4 mfma_bf(const bf16x8 a, const bf16x8 b, const f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// acc += A * B for one K = 32 chunk from the split planes {hi, mid, lo} of both operands: the six partial products of
// weight >= 2^-16, the small ones first.  The ONE place the product set is written down: the dense 3x3, de_convs.3 and
// the device self test (gtcrn_selftest_split3, tests/test_gpu_parity.py) all go through it.
__device__ __forceinline__ f32x4 split_mm6(const bf16x8 (&ap)[3], const bf16x8 (&bp)[3], f32x4 acc) {
    acc = mfma_bf(ap[0], bp[2], acc);
    acc = mfma_bf(ap[2], bp[0], acc);
    acc = mfma_bf(ap[1], bp[1], acc);
    acc = mfma_bf(ap[0], bp[1], acc);
    acc = mfma_bf(ap[1], bp[0], acc);
    acc = mfma_bf(ap[0], bp[0], acc);
    return acc;
}
// The int8 / fp16 variant (Q) takes the same road with ONE plane: its activations are fp16 numbers, so h lives in LDS as
// fp16 records (the first 32 bytes of the 96-byte record) and the dense 3x3 is five v_mfma_f32_16x16x32_f16 per tile --
// no conversion per matrix instruction (round 2 kept fp32 records and converted both operands at every one of nine
// 16x16x16 instructions).  The weights are the packer's fp16 K-chunk matrices (pack.cpp quantize_packed).
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void st_half(float* img, int rec, int g, const f32x4 v) {
    *reinterpret_cast<h16x4*>(img + rec + 2 * g) = to_h4(v);
}
__device__ __forceinline__ f32x4 ld_half(const float* img, int rec, int g) {
    const h16x4 h = *reinterpret_cast<const h16x4*>(img + rec + 2 * g);
    f32x4 r = {(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
    return r;
}
// record format of a dense block's h image
enum ImgFmt { IMG_F32 = 0, IMG_SPLIT3 = 1, IMG_HALF = 2 };

// Hand-off tensors (en0..en4, gtcn1, gtcn2+en4) in HBM: fp32 records, or -- in the Q variant, whose activations are
// fp16 numbers anyway -- fp16 records of half the size in the same buffers (element offsets are unchanged: the
// kernels index through a pointer of the element type).
template <bool Q> struct HandOff { using t = float; };
template <> struct HandOff<true> { using t = _Float16; };
template <bool Q>
__device__ __forceinline__ f32x4 ldx(const typename HandOff<Q>::t* p) {
    if constexpr (Q) {
        const h16x4 h = *reinterpret_cast<const h16x4*>(p);
        f32x4 r = {(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
        return r;
    } else {
        return ld4(p);
    }
}
template <bool Q, bool NT = true>
__device__ __forceinline__ void stx(typename HandOff<Q>::t* p, const f32x4 v) {
    // written once, read once by a later kernel, far larger than the caches: streaming (nontemporal) stores
    if constexpr (NT) {
        if constexpr (Q) __builtin_nontemporal_store(to_h4(v), reinterpret_cast<h16x4*>(p));
        else __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p));
    } else {
        if constexpr (Q) *reinterpret_cast<h16x4*>(p) = to_h4(v);
        else st4(p, v);
    }
}
// (Also for the tensors the very next kernel reads: leaving those to the caches measured 1.5 % slower on that reader.)

// Diagnostic build only (-DGT_STAMPS, libgtcrn_micro_hip_stamps.so): s_memtime stamps at the
// barrier-delimited phases, summed per workgroup and written to a buffer nothing else reads.
// In the product build these macros expand to nothing.
#ifdef GT_STAMPS
struct Stamps {
    unsigned long long t, acc[16];
};
#define STAMP_INIT(S)                                   \
    Stamps S;                                           \
    _Pragma("unroll") for (int k_ = 0; k_ < 16; ++k_) S.acc[k_] = 0; \
    S.t = __builtin_amdgcn_s_memtime();
#define STAMP(S, k)                                                  \
    {                                                                \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
        S.acc[k] += now_ - S.t;                                      \
        S.t = now_;                                                  \
    }
#define STAMP_OUT(S, ptr)                                                                       \
    if (ptr && threadIdx.x == 0) {                                                              \
        _Pragma("unroll") for (int k_ = 0; k_ < 16; ++k_) ptr[(long)blockIdx.x * 16 + k_] = S.acc[k_]; \
    }
// (a workgroup that returns before STAMP_INIT -- the indexed stream kernels, no rows this call -- reports zeros, not the
// previous launch's record)
#define STAMP_ZERO(ptr)                                                                         \
    if (ptr && threadIdx.x == 0) {                                                              \
        _Pragma("unroll") for (int k_ = 0; k_ < 16; ++k_) ptr[(long)blockIdx.x * 16 + k_] = 0; \
    }
#define STAMP_PARAM , Stamps& SS
#define STAMP_ARG , SS
#else
#define STAMP_INIT(S)
#define STAMP(S, k)
#define STAMP_OUT(S, ptr)
#define STAMP_ZERO(ptr)
#define STAMP_PARAM
#define STAMP_ARG
#endif

struct Lane {
    int tid, lane, wave, n, g;
};
__device__ __forceinline__ Lane lane_info() {
    Lane L;
    L.tid = threadIdx.x;
    L.lane = L.tid & 63;
    L.wave = __builtin_amdgcn_readfirstlane(L.tid >> 6);
    L.n = L.lane & 15;
    L.g = L.lane >> 4;
    return L;
}

// =============================================================================== STFT
// torch.stft(x,512,256,512,win,center=True,reflect,onesided) (infer.py:60-67): frame t =
// reflect_pad(x,256)[256t : 256t+512] * win, unnormalised rFFT.  One wave per frame: the 512 real
// samples are packed as 256 complex, radix-4 Stockham FFT in LDS, then the real-FFT split.
// The stage itself (tables, window, fft256, split, merge, envelope, frame fetch) is fft256.h.
constexpr int FFT_WAVES = 4;

// ADJ = true: the adjoint of k_istft's linear map (the backward of torch.istft, used by the fused HybridLoss):
// frames are cut from the ZERO-padded signal, every bin is scaled by c_k / 512 (c_k = 2 except DC and Nyquist: the
// c2r transform reads those once) and the result is ADDED to `spec`.
template <bool ADJ>
__global__ __launch_bounds__(FFT_WAVES * 64) void k_stft(const float* __restrict__ wave, int B, long L, int T,
                                                        const int* __restrict__ lens,
                                                        const float* __restrict__ win,
                                                        const float2* __restrict__ twid, float* __restrict__ spec,
                                                        long sb, long sf, long st, float* __restrict__ frames_out) {
    __shared__ float2 s_tw[256];
    __shared__ float2 s_tw512[256];
    __shared__ float s_win[512];
    __shared__ float2 s_buf[FFT_WAVES][2][256];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    fft_tables_load(s_tw, s_tw512, s_win, twid, win, tid, FFT_WAVES * 64);
    __syncthreads();
    const long nframes = (long)B * T;
    const long base = (long)blockIdx.x * (FFT_WAVES * FRAMES_PER_WAVE);
    // samples of a frame (frame_fetch): only the first and the last two frames of an utterance touch the edges.
    // lens (optional): utterance b holds lens[b] <= L samples in its row of L (variable-length batch); its frames
    // t >= 1 + lens[b]/256 do not exist (nothing is stored for them) and its reflected edge is its own
    auto fetch = [&](long fr, float2 (&v)[4]) {
        bool live = fr < nframes;
        const int b = live ? (int)(fr / T) : 0;
        int t = live ? (int)(fr - (long)b * T) : 0;
        const float* x = wave + (long)b * L;
        const long Lb = lens ? (long)lens[b] : L;
        if (t > (int)(Lb >> 8)) t = 0;                        // a frame past the utterance's end: not live, reads frame 0
        if constexpr (!ADJ) {
            frame_fetch(x, t, Lb, lane, v);
        } else {                                              // frame_fetch's two paths, zeros where it reflects
            const long lo = 256L * t - 256;
            if (lo >= 0 && lo + 512 <= Lb && ((reinterpret_cast<uintptr_t>(x + lo) & 7) == 0)) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const float2*>(x + lo + 2 * (lane + 64 * q));
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const long i0 = 256L * t + 2 * (lane + 64 * q);
                    const long j0 = i0 - 256, j1 = j0 + 1;
                    v[q] = make_float2(j0 >= 0 && j0 < Lb ? x[j0] : 0.f, j1 >= 0 && j1 < Lb ? x[j1] : 0.f);
                }
            }
        }
    };
    float2 cur[4], nxt[4];
    fetch(base + wv, cur);
    for (int it = 0; it < FRAMES_PER_WAVE; ++it) {
        // all 4 waves run the same number of iterations
        const long fr = base + (long)it * FFT_WAVES + wv;
        bool live = fr < nframes;
        const int b = live ? (int)(fr / T) : 0;
        const int t = live ? (int)(fr - (long)b * T) : 0;
        if (lens && live && t > (lens[b] >> 8)) live = false;
        float2* A = s_buf[wv][0];
        float2* Bf = s_buf[wv][1];
        if (it + 1 < FRAMES_PER_WAVE) fetch(fr + FFT_WAVES, nxt);   // next frame's samples: in flight during this FFT
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int m = lane + 64 * q;
            const float2 v = frame_window(cur[q], s_win, m);
            A[m] = v;
            if (frames_out && live) {
                frames_out[fr * 512 + 2 * m] = v.x;
                frames_out[fr * 512 + 2 * m + 1] = v.y;
            }
        }
        wave_lds_sync();
        fft256<-1>(A, Bf, s_tw, lane);
        if (live && spec) {
            float* o = spec + (long)b * sb + (long)t * st;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = lane + 64 * q;
                const float2 zk = A[k], X = rfft_bin(A, s_tw512, k, zk);
                // the re/im pair is contiguous and 8-byte aligned (even strides): one 8-byte store
                float2* ok = reinterpret_cast<float2*>(o + (long)k * sf);
                float2* on = reinterpret_cast<float2*>(o + 256L * sf);
                if (ADJ) {
                    const float ck = (k == 0 ? 1.0f : 2.0f) / 512.0f;
                    const float2 old = *ok;
                    *ok = make_float2(old.x + ck * X.x, old.y + (k == 0 ? 0.f : ck * X.y));
                    if (k == 0) { const float2 o2 = *on; *on = make_float2(o2.x + rfft_nyquist(zk).x * (1.0f / 512.0f), o2.y); }
                } else {
                    *ok = X;
                    if (k == 0) *on = rfft_nyquist(zk);
                }
            }
        }
        wave_lds_sync();
#pragma unroll
        for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
    }
}

// Attenuation limit (include/gtcrn_micro_hip.h, "attenuation limit"): dry gain g, dry sample x, wet sample w ->
// fl(fl(g x) + fl(fl(1 - g) w)).  Four fp32 roundings, each in a call of its own: -ffp-contract=on fuses inside one source
// expression only, so no fma is formed and numpy float32 reproduces the value bit for bit.  g = 0 gives w, g = 1 gives x.
__device__ __forceinline__ float wave_mix(float g, float x, float w) {
    return __fadd_rn(__fmul_rn(g, x), __fmul_rn(__fsub_rn(1.0f, g), w));
}

// torch.istft(view_as_complex(y),512,256,512,win) (infer.py:73-76): irfft (1/512), * win,
// overlap-add, / sum(win^2), trim 256 samples at both ends -> 256*(T-1) samples.  The 512-point
// c2r runs as a 256-point complex inverse FFT of the merged spectrum (scale 1/256).
// One workgroup produces ISTFT_BLOCKS hop blocks of one utterance from ISTFT_BLOCKS+1 frames.
// The body of k_istft and of its sibling k_istft_mix (MIX: the attenuation limit of the offline calls -- the stored sample
// becomes wave_mix(gain[b], dry[b][n], sample), dry = the call's input wave in rows of dry_stride samples, sample n of the
// output aligned with sample n of the input; a thread's dry samples, one per hop block, are fetched with the first frame,
// ahead of the transforms).
template <bool MIX>
__device__ __forceinline__ void istft_body(const float* __restrict__ spec, long sb, long sf, long st, int B, int T,
                                           const int* __restrict__ lens, const float* __restrict__ win,
                                           const float2* __restrict__ twid, float* __restrict__ wave,
                                           const float* __restrict__ dry, long dry_stride, const float* __restrict__ gain) {
    __shared__ float2 s_tw[256];
    __shared__ float2 s_tw512[256];
    __shared__ float s_win[512];
    // every frame keeps its own FFT buffer: the inverse transform ends there and is windowed IN PLACE, so the
    // overlap-add reads the frames where they are (no second 16 KB frame image: 30 KB per workgroup, five per CU
    // instead of four -- the kernel is latency bound on its spectrogram reads: -5.5 %)
    __shared__ float2 s_fa[ISTFT_BLOCKS + 1][256];
    __shared__ float2 s_fb[FFT_WAVES][256];
    float (*s_fr)[512] = reinterpret_cast<float (*)[512]>(&s_fa[0][0]);
    static_assert(ISTFT_BLOCKS + 1 <= 2 * FFT_WAVES, "one buffer per frame of the two rounds");
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    fft_tables_load(s_tw, s_tw512, s_win, twid, win, tid, FFT_WAVES * 64);
    __syncthreads();
    const int groups = (T - 1 + ISTFT_BLOCKS - 1) / ISTFT_BLOCKS;
    const int b = blockIdx.x / groups, grp = blockIdx.x - b * groups;
    const int nblk = lens ? (lens[b] >> 8) : T - 1;           // hop blocks of this utterance (T_b - 1)
    const int j0 = grp * ISTFT_BLOCKS;                        // first hop block == first frame needed
    if (j0 >= nblk) return;                                   // variable-length batch: past this utterance's end
    const int nfr = min(ISTFT_BLOCKS, nblk - j0) + 1;
    constexpr int ROUNDS = (ISTFT_BLOCKS + 1 + FFT_WAVES - 1) / FFT_WAVES;
    // bins k and 256-k of a frame (k = lane + 64 q); the next round's are fetched before this round's FFT
    auto fetch = [&](int it, float2 (&vk)[4], float2 (&vm)[4]) {
        const int fi = it * FFT_WAVES + wv;
        const int t = j0 + (fi < nfr ? fi : 0);
        const float* x = spec + (long)b * sb + (long)t * st;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = lane + 64 * q;
            vk[q] = *reinterpret_cast<const float2*>(x + (long)k * sf);
            vm[q] = *reinterpret_cast<const float2*>(x + (long)(256 - k) * sf);
        }
    };
    float2 ck[4], cm[4], nk[4], nm[4];
    fetch(0, ck, cm);
    static_assert(FFT_WAVES * 64 == 256, "the overlap-add below: one hop block per pass, thread = sample");
    float dv[ISTFT_BLOCKS];
    if constexpr (MIX) {
        const float* x = dry + (long)b * dry_stride + (long)j0 * 256 + tid;
#pragma unroll
        for (int jb = 0; jb < ISTFT_BLOCKS; ++jb) dv[jb] = jb < nfr - 1 ? x[jb * 256] : 0.f;
    }
    for (int it = 0; it < ROUNDS; ++it) {
        const int fi = it * FFT_WAVES + wv;
        const bool live = fi < nfr;
        float2* A = s_fa[fi < ISTFT_BLOCKS + 1 ? fi : ISTFT_BLOCKS];
        float2* Bf = s_fb[wv];
        if (it + 1 < ROUNDS) fetch(it + 1, nk, nm);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = lane + 64 * q;
            A[k] = irfft_bin(ck[q], cm[q], s_tw512, k);
        }
        wave_lds_sync();
        fft256<1>(A, Bf, s_tw, lane);
        if (live) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int m = lane + 64 * q;
                const float2 f = irfft_window(A[m], s_win, m);
                s_fr[fi][2 * m] = f.x;
                s_fr[fi][2 * m + 1] = f.y;
            }
        }
        wave_lds_sync();
#pragma unroll
        for (int q = 0; q < 4; ++q) { ck[q] = nk[q]; cm[q] = nm[q]; }
    }
    __syncthreads();   // the windowed frames of all four waves are overlap-added below
    // overlap-add: output block j = frame j second half + frame j+1 first half
    float* o = wave + (long)b * 256 * (T - 1);                // rows of 256 (T - 1) samples
    if constexpr (MIX) {
        const float g = gain[b];
        const float env = ola_env(s_win, tid);
#pragma unroll
        for (int jb = 0; jb < ISTFT_BLOCKS; ++jb) {
            if (jb >= nfr - 1) break;
            const float acc = s_fr[jb][256 + tid] + s_fr[jb + 1][tid];
            o[(long)(j0 + jb) * 256 + tid] = wave_mix(g, dv[jb], ola_div(acc, env));
        }
        return;
    }
    for (int idx = tid; idx < (nfr - 1) * 256; idx += FFT_WAVES * 64) {
        const int jb = idx >> 8, i = idx & 255;
        const float acc = s_fr[jb][256 + i] + s_fr[jb + 1][i];
        o[(long)(j0 + jb) * 256 + i] = ola_div(acc, ola_env(s_win, i));
    }
}
__global__ __launch_bounds__(FFT_WAVES * 64) void k_istft(const float* __restrict__ spec, long sb, long sf, long st,
                                                         int B, int T, const int* __restrict__ lens,
                                                         const float* __restrict__ win,
                                                         const float2* __restrict__ twid, float* __restrict__ wave) {
    istft_body<false>(spec, sb, sf, st, B, T, lens, win, twid, wave, nullptr, 0, nullptr);
}
__global__ __launch_bounds__(FFT_WAVES * 64) void k_istft_mix(const float* __restrict__ spec, long sb, long sf, long st,
                                                             int B, int T, const int* __restrict__ lens,
                                                             const float* __restrict__ win,
                                                             const float2* __restrict__ twid, float* __restrict__ wave,
                                                             const float* __restrict__ dry, long dry_stride,
                                                             const float* __restrict__ gain) {
    istft_body<true>(spec, sb, sf, st, B, T, lens, win, twid, wave, dry, dry_stride, gain);
}

// ---- stream slots (k_stream_ms_slots and the IDX = true instantiations of k_stream_wide / k_wave_analysis / k_wave_synthesis)
// The states of all resident streams stay where they are; a call names, in a device array, the slots that step, and a device
// word says how many of them: row i of the call (its spectrum / sample rows are compact) is the stream whose state sits in
// slot slots[i].  One captured graph then serves a changing active set.  The contiguous kernels are the IDX = false
// instantiations of the same kernels: there the row map is `sidx * ST_FLOATS` and the two trailing arguments are not read.
__device__ __forceinline__ int slot_count(const int* __restrict__ cnt, int max_active) {
    return cnt ? min(max(*cnt, 0), max_active) : max_active;     // rows at or beyond it are neither read nor written
}
// The stream kernels read their workgroup's slot ids once, into SLOT_WORDS LDS words behind the kernel's images (rows past
// nlive repeat the last live one, so the clamped "valid record" addresses of dead lanes stay inside a slot this call owns);
// one barrier, before anything else is issued, publishes them.  SROW(sidx) = floats from stb to the state of the
// workgroup's row sidx: a lane reads its row's word where it forms the address (nothing is kept live across the phases);
// in the contiguous form the expression it always was (defined in front of k_stream_ms, undefined after k_stream_wide).
constexpr int SLOT_WORDS = 8;

// ===================================================================== hop-level waveform streaming
// The caller's torch.stft -> model loop -> torch.istft at one 256-sample hop per call (include/gtcrn_micro_hip.h,
// gtcrn_wave_stream_step).  Frame t of torch.stft(center=True) is x[256t-256 : 256t+256]: at call k the library
// frames hop k (with hop k-1 from the stream's input ring), the model steps it, and the synthesis emits hop block k-1
// = second half of frame k-1 (the stored tail) + first half of frame k, / env.  Frame 0 is the start-reflected hop 0
// whose one future sample, x[256], meets win[0] == 0 (it is read as 0).  The arithmetic is k_stft / k_front's and
// k_istft's because it is the same functions (fft256.h: frame_window, fft256<-1>, rfft_bin, rfft_nyquist; irfft_bin,
// fft256<1>, irfft_window, ola_div), so the stream equals gtcrn_forward_wave one hop late, bit for bit.
// Samples are float or int16 (pcm16_widen / pcm16_round, which the PCM16 kernels call too).
// FLUSH: the stream's last frame from the ring and r < 256 extra samples, end-reflected as reflect_idx does.
// The packet kernels also take G.711 codes (g711u / g711a, kernels.h): read as D_law[c] / 32768, stored as E_law of the
// int16 the PCM16 store would have written -- integer arithmetic in registers, no table.
template <typename S>
inline constexpr bool is_g711 = std::is_same<S, g711u>::value || std::is_same<S, g711a>::value;
template <typename S>
__device__ __forceinline__ float wave_ld(const S* p) {
    if constexpr (std::is_same<S, short>::value) return pcm16_widen(*p);
    else if constexpr (is_g711<S>) return pcm16_widen(g711_decode(S::law, p->code));
    else return *p;
}
template <typename S>
__device__ __forceinline__ void wave_st(S* p, float y) {
    if constexpr (std::is_same<S, short>::value) *p = (short)pcm16_round(y);
    else if constexpr (is_g711<S>) p->code = (unsigned char)g711_encode(S::law, pcm16_round(y));
    else *p = y;
}

// One wave per (stream, hop) frame, WAVE_FRAMES frames per wave.  Reads the wave state, writes none of it (the
// synthesis advances it, after the model step, on the same stream): frame-major spectra (N, nhops, 257, 2).
// IDX (the indexed instantiations, one hop per call): row n of the call is the stream in slot slots[n] -- its wave state and, in the
// synthesis, its dry gain are read there, the sample and spectrum rows stay compact; N is the clamped device count.
template <typename S, bool FLUSH, bool IDX = false>
__global__ __launch_bounds__(FFT_WAVES * 64) void k_wave_analysis(const S* __restrict__ in, long in_stride, int N,
                                                                 int nhops, int r, const float* __restrict__ wstate,
                                                                 const float* __restrict__ win,
                                                                 const float2* __restrict__ twid,
                                                                 float* __restrict__ spec, const int* __restrict__ slots,
                                                                 const int* __restrict__ cnt) {
    if constexpr (IDX) N = slot_count(cnt, N);
    __shared__ float2 s_tw[256];
    __shared__ float2 s_tw512[256];
    __shared__ float s_win[512];
    __shared__ float2 s_buf[FFT_WAVES][2][256];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    fft_tables_load(s_tw, s_tw512, s_win, twid, win, tid, FFT_WAVES * 64);
    __syncthreads();
    const long nframes = (long)N * nhops;
    const long base = (long)blockIdx.x * (FFT_WAVES * WAVE_FRAMES);
    for (int it = 0; it < WAVE_FRAMES; ++it) {
        const long fr = base + (long)it * FFT_WAVES + wv;
        if (fr >= nframes) break;                                  // (wave uniform; no workgroup barrier follows)
        const int n = (int)(fr / nhops), h = (int)(fr - (long)n * nhops);
        const float* ws = wstate + (long)(IDX ? slots[n] : n) * WS_FLOATS;
        const int t = *reinterpret_cast<const int*>(ws + WS_CNT) + h;
        const S* x = in + (long)n * in_stride;
        float2* A = s_buf[wv][0];
        float2* Bf = s_buf[wv][1];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int m = lane + 64 * q;
            float2 c;
            if constexpr (FLUSH) {
                // [ring (last 512 samples) ++ tail (r samples)]: sample i of frame t sits at 256 + i, reflected at the end
                const int rl = 512 + r;
                int i0 = 256 + 2 * m, i1 = i0 + 1;
                i0 = i0 >= rl ? 2 * (rl - 1) - i0 : i0;
                i1 = i1 >= rl ? 2 * (rl - 1) - i1 : i1;
                c.x = i0 < 512 ? ws[WS_RING + i0] : wave_ld(x + (i0 - 512));
                c.y = i1 < 512 ? ws[WS_RING + i1] : wave_ld(x + (i1 - 512));
            } else if (t == 0) {
                // frame 0 = [x[256], x[255..1], x[0..255]]; x[256] is not here yet and meets win[0] == 0
                if (q < 2) {
                    const int i0 = 256 - 2 * m;
                    c.x = i0 < 256 ? wave_ld(x + (i0 < 256 ? i0 : 255)) : 0.f;
                    c.y = wave_ld(x + (i0 - 1));
                } else {
                    c.x = wave_ld(x + (2 * m - 256));
                    c.y = wave_ld(x + (2 * m - 255));
                }
            } else if (q < 2) {
                // the previous hop: the ring's newest 256 samples, or hop h - 1 of this call
                if (h == 0) c = *reinterpret_cast<const float2*>(ws + WS_RING + 256 + 2 * m);
                else c = make_float2(wave_ld(x + 256L * (h - 1) + 2 * m), wave_ld(x + 256L * (h - 1) + 2 * m + 1));
            } else {
                c = make_float2(wave_ld(x + 256L * h + 2 * m - 256), wave_ld(x + 256L * h + 2 * m - 255));
            }
            A[m] = frame_window(c, s_win, m);
        }
        wave_lds_sync();
        fft256<-1>(A, Bf, s_tw, lane);
        float* o = spec + fr * 514;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = lane + 64 * q;
            const float2 zk = A[k];
            *reinterpret_cast<float2*>(o + 2 * k) = rfft_bin(A, s_tw512, k, zk);
            if (k == 0) *reinterpret_cast<float2*>(o + 512) = rfft_nyquist(zk);
        }
        wave_lds_sync();
    }
}

// One wave per stream, its hops in order: merge, inverse FFT, window and / 256 as k_istft; the overlap-add runs in
// registers (lane's first-half samples 2m, 2m+1, m = lane + 64 q, q < 2, meet the previous frame's 256 + 2m, 256 + 2m + 1,
// which the same lane holds at q + 2).  Then the state advances: tail, input ring (last 512 samples), hop counter.
// FLUSH emits the stream's last block and leaves the wave state as it is (the stream has ended).  MODE: Synth (kernels.h).
// wave_sum / wave_max: every lane ends with the same value, the xor butterfly over lane distances 1, 2, 4, 8, 16, 32 in
// that order (an fp32 add is commutative, so both partners of a step round alike).
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = __fadd_rn(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = fmaxf(v, __shfl_xor(v, d));
    return v;
}
// wave_sum's value -- the same pairwise additions, so the same bits -- as a wave-uniform scalar and without the LDS crossbar
// (the Guard mode runs twenty of these per block).  All 64 lanes must be active.  After the steps over distances 1 and 2
// (quad permutes) the four lanes of a quad hold one value, so the half-row mirror hands lane l what lane l ^ 4 holds, and
// after that step the row mirror what lane l ^ 8 holds; the four rows' sums are then read as scalars and added as lane 0's
// butterfly adds them, (r0 + r1) + (r2 + r3).
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float wave_sum_uniform(float v) {
    v = __fadd_rn(v, dpp_f32<0xB1>(v));       // quad_perm [1, 0, 3, 2]
    v = __fadd_rn(v, dpp_f32<0x4E>(v));       // quad_perm [2, 3, 0, 1]
    v = __fadd_rn(v, dpp_f32<0x141>(v));      // row_half_mirror
    v = __fadd_rn(v, dpp_f32<0x140>(v));      // row_mirror
    const auto row = [&](int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); };
    return __fadd_rn(__fadd_rn(row(0), row(16)), __fadd_rn(row(32), row(48)));
}
template <typename S, bool FLUSH, bool IDX, Synth MODE>
__global__ __launch_bounds__(FFT_WAVES * 64) void k_wave_synthesis(const float* __restrict__ spec, const S* __restrict__ in,
                                                                  long in_stride, S* __restrict__ out, long out_stride,
                                                                  int N, int nhops, int r, float* __restrict__ wstate,
                                                                  const float* __restrict__ win,
                                                                  const float2* __restrict__ twid,
                                                                  const float* __restrict__ gain,
                                                                  const int* __restrict__ slots,
                                                                  const int* __restrict__ cnt,
                                                                  float* __restrict__ meters,
                                                                  float* __restrict__ ramp,
                                                                  float* __restrict__ alc,
                                                                  const float* __restrict__ alc_params,
                                                                  float* __restrict__ tone,
                                                                  const float* __restrict__ tone_params,
                                                                  const float* __restrict__ tone_table) {
    constexpr bool GUARD = MODE == Synth::Guard;
    constexpr bool MIX = MODE == Synth::Mix || MODE == Synth::MixRamp, METER = MODE == Synth::Meter || MODE == Synth::MeterRamp;
    constexpr bool RAMP = MODE == Synth::MixRamp || MODE == Synth::MeterRamp, ALC = MODE == Synth::Alc;
    if constexpr (IDX) N = slot_count(cnt, N);
    __shared__ float2 s_tw[256];
    __shared__ float2 s_tw512[256];
    __shared__ float s_win[512];
    __shared__ float2 s_buf[FFT_WAVES][2][256];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    fft_tables_load(s_tw, s_tw512, s_win, twid, win, tid, FFT_WAVES * 64);
    __syncthreads();
    const int n = blockIdx.x * FFT_WAVES + wv;
    if (n >= N) return;
    const long slot = IDX ? slots[n] : n;                          // the stream's place in wstate and gain
    float* ws = wstate + slot * WS_FLOATS;
    const int c0 = *reinterpret_cast<const int*>(ws + WS_CNT);
    // a flush of a stream that holds fewer than 257 samples has no block (gtcrn_forward_wave rejects such a clip)
    const bool none = FLUSH && 256L * c0 + r < 257;
    float2 prev[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) prev[q] = *reinterpret_cast<const float2*>(ws + WS_TAIL + 2 * (lane + 64 * q));
    float env[2][2];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            env[q][e] = ola_env(s_win, 2 * (lane + 64 * q) + e);
        }
    float2* A = s_buf[wv][0];
    float2* Bf = s_buf[wv][1];
    S* o = out + (long)n * out_stride;
    float g = 0.f;
    float2 dry0[2];      // MIX: the ring's newest 256 samples, this lane's pairs
    if constexpr (MIX) {
        g = gain[slot];
#pragma unroll
        for (int q = 0; q < 2; ++q) dry0[q] = *reinterpret_cast<const float2*>(ws + WS_RING + 256 + 2 * (lane + 64 * q));
    }
    float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);      // METER: the stream's record, the same in every lane
    float pk = 0.f;                                    // METER: this lane's max |y| over the call (a max is exact in any order)
    if constexpr (METER) {
        if (gain) g = gain[slot];
#pragma unroll
        for (int q = 0; q < 2; ++q) dry0[q] = *reinterpret_cast<const float2*>(ws + WS_RING + 256 + 2 * (lane + 64 * q));
        rec = *reinterpret_cast<const float4*>(meters + 4 * slot);
    }
    float p = 0.f;       // RAMP: the gain the stream's last block ended at (loaded here, first read behind hop 0's transform)
    if constexpr (RAMP) p = ramp[slot];
    float4 av[5];        // ALC: the record's two halves and parameter words 0 .. 11, as loaded (every lane the same address)
    AlcParams P;         // ALC: both made scalars behind hop 0's transform
    AlcRecord R;
    if constexpr (ALC) {
        if (gain) g = gain[slot];
        if (gain && ramp) p = ramp[slot];
#pragma unroll
        for (int q = 0; q < 2; ++q) dry0[q] = *reinterpret_cast<const float2*>(ws + WS_RING + 256 + 2 * (lane + 64 * q));
        if (meters) rec = *reinterpret_cast<const float4*>(meters + 4 * slot);
        av[0] = *reinterpret_cast<const float4*>(alc + 8 * slot);
        av[1] = *reinterpret_cast<const float4*>(alc + 8 * slot + 4);
#pragma unroll
        for (int q = 0; q < 3; ++q) av[2 + q] = *reinterpret_cast<const float4*>(alc_params + 4 * q);
    }
    float4 tv[5];        // GUARD: the tone record's two halves and parameter words 0 .. 11, as loaded
    ToneParams TP;       // GUARD: both made scalars behind hop 0's transform
    ToneRecord TR;
    if constexpr (GUARD) {
        if (gain) g = gain[slot];
        if (gain && ramp) p = ramp[slot];
#pragma unroll
        for (int q = 0; q < 2; ++q) dry0[q] = *reinterpret_cast<const float2*>(ws + WS_RING + 256 + 2 * (lane + 64 * q));
        if (meters) rec = *reinterpret_cast<const float4*>(meters + 4 * slot);
        if (alc) {
            av[0] = *reinterpret_cast<const float4*>(alc + 8 * slot);
            av[1] = *reinterpret_cast<const float4*>(alc + 8 * slot + 4);
#pragma unroll
            for (int q = 0; q < 3; ++q) av[2 + q] = *reinterpret_cast<const float4*>(alc_params + 4 * q);
        }
        tv[0] = *reinterpret_cast<const float4*>(tone + 8 * slot);
        tv[1] = *reinterpret_cast<const float4*>(tone + 8 * slot + 4);
#pragma unroll
        for (int q = 0; q < 3; ++q) tv[2 + q] = *reinterpret_cast<const float4*>(tone_params + 4 * q);
    }
    for (int h = 0; h < nhops; ++h) {
        const float* x = spec + ((long)n * nhops + h) * 514;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = lane + 64 * q;
            A[k] = irfft_bin(*reinterpret_cast<const float2*>(x + 2 * k), *reinterpret_cast<const float2*>(x + 2 * (256 - k)),
                             s_tw512, k);
        }
        wave_lds_sync();
        fft256<1>(A, Bf, s_tw, lane);
        float2 f[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int m = lane + 64 * q;
            f[q] = irfft_window(A[m], s_win, m);
        }
        wave_lds_sync();     // A is rewritten by the next hop's merge
        const bool zero = none || c0 + h == 0;     // call 0 of a stream emits zeros (the one-hop delay)
        if constexpr (ALC) {
            if (h == 0) {      // (made scalars HERE, as the ramp words below)
                const auto sc = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
                p = sc(p);
                g = sc(g);
                R = AlcRecord{sc(av[0].x), sc(av[0].y), sc(av[0].z), sc(av[0].w), sc(av[1].x), sc(av[1].y)};
                P = AlcParams{sc(av[2].x), sc(av[2].y), sc(av[2].z), sc(av[2].w), sc(av[3].x), sc(av[3].y),
                              sc(av[3].z), sc(av[3].w), sc(av[4].x), sc(av[4].y), sc(av[4].z)};
            }
            const bool ramps = h == 0 && gain && ramp && p != g;      // this block mixes with gain_ramp_at(p, g, i)
            float wq[2][2], xq[2][2], mq[2][2], yq[2][2];                // sample 2 (lane + 64 q) + e of the block
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int m = lane + 64 * q;
                float2 d = dry0[q];
                if (h > 0) {
                    const S* xd = in + (long)n * in_stride + 256L * (h - 1) + 2 * m;
                    d = make_float2(wave_ld(xd), wave_ld(xd + 1));
                }
                xq[q][0] = d.x;
                xq[q][1] = d.y;
                wq[q][0] = ola_div(prev[q].x + f[q].x, env[q][0]);
                wq[q][1] = ola_div(prev[q].y + f[q].y, env[q][1]);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const float ge = ramps ? gain_ramp_at(p, g, 2 * m + e) : g;
                    mq[q][e] = gain ? wave_mix(ge, xq[q][e], wq[q][e]) : wq[q][e];
                    yq[q][e] = 0.f;
                }
                prev[q] = f[q + 2];
            }
            float ex = 0.f;
            if (zero) {
                if (!none) R = AlcRecord{1.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            } else {
                const float ew = wave_sum(alc_lane_sum(wq[0][0], wq[0][1], wq[1][0], wq[1][1]));
                ex = wave_sum(alc_lane_sum(xq[0][0], xq[0][1], xq[1][0], xq[1][1]));
                const float pm = wave_max(fmaxf(fmaxf(fabsf(mq[0][0]), fabsf(mq[0][1])), fmaxf(fabsf(mq[1][0]), fabsf(mq[1][1]))));
                float a0, a1;
                alc_decide(P, R, ew, ex, pm, a0, a1);
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int e = 0; e < 2; ++e) yq[q][e] = __fmul_rn(gain_ramp_at(a0, a1, 2 * (lane + 64 * q) + e), mq[q][e]);
            }
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                wave_st(o + 256L * h + 2 * (lane + 64 * q), yq[q][0]);
                wave_st(o + 256L * h + 2 * (lane + 64 * q) + 1, yq[q][1]);
            }
            if (meters) {      // the meters see y; their E_dry is E_x (the same sums in the same order; 0 for a zero block)
                rec.x = __fadd_rn(rec.x, ex);
                rec.y = __fadd_rn(rec.y, wave_sum(alc_lane_sum(yq[0][0], yq[0][1], yq[1][0], yq[1][1])));
                rec.w = __fadd_rn(rec.w, 1.0f);
                pk = fmaxf(pk, fmaxf(fmaxf(fabsf(yq[0][0]), fabsf(yq[0][1])), fmaxf(fabsf(yq[1][0]), fabsf(yq[1][1]))));
            }
            continue;
        }
        if constexpr (GUARD) {
            const auto sc = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
            if (h == 0) {      // (made scalars HERE, as the ramp words below)
                p = sc(p);
                g = sc(g);
                if (alc) {
                    R = AlcRecord{sc(av[0].x), sc(av[0].y), sc(av[0].z), sc(av[0].w), sc(av[1].x), sc(av[1].y)};
                    P = AlcParams{sc(av[2].x), sc(av[2].y), sc(av[2].z), sc(av[2].w), sc(av[3].x), sc(av[3].y),
                                  sc(av[3].z), sc(av[3].w), sc(av[4].x), sc(av[4].y), sc(av[4].z)};
                }
                TR = ToneRecord{sc(tv[0].x), sc(tv[0].y), sc(tv[0].z), sc(tv[0].w), sc(tv[1].x), sc(tv[1].y), sc(tv[1].z), sc(tv[1].w)};
                TP = ToneParams{sc(tv[2].x), sc(tv[2].y), sc(tv[2].z), sc(tv[2].w), sc(tv[3].x), sc(tv[3].y),
                                sc(tv[3].z), sc(tv[3].w), sc(tv[4].x), sc(tv[4].y), sc(tv[4].z)};
            }
            float wq[2][2], xq[2][2], mq[2][2], yq[2][2];                // sample 2 (lane + 64 q) + e of the block
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int m = lane + 64 * q;
                float2 d = dry0[q];
                if (h > 0) {
                    const S* xd = in + (long)n * in_stride + 256L * (h - 1) + 2 * m;
                    d = make_float2(wave_ld(xd), wave_ld(xd + 1));
                }
                xq[q][0] = d.x;
                xq[q][1] = d.y;
                wq[q][0] = ola_div(prev[q].x + f[q].x, env[q][0]);
                wq[q][1] = ola_div(prev[q].y + f[q].y, env[q][1]);
                prev[q] = f[q + 2];
            }
            float ex = 0.f;
            bool dry = false;      // this block is passed dry
            const bool zs = __builtin_amdgcn_readfirstlane((int)zero) != 0;      // zero as a scalar: the records' branches stay scalar
            if (zs) {
                if (!none) {
                    TR = ToneRecord{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    if (alc) R = AlcRecord{1.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                }
            } else {
                ex = wave_sum(alc_lane_sum(xq[0][0], xq[0][1], xq[1][0], xq[1][1]));
                float Pf[TONE_FREQS];
                // (the table's address is made opaque HERE: hoisted over the transform, the twenty loads hold 80 registers there)
                typedef float f4 __attribute__((ext_vector_type(4)));
                const float* tt = tone_table;
                asm volatile("" : "+s"(tt));
                const auto* tg = (const __attribute__((address_space(1))) float*)tt;
#pragma unroll
                for (int k = 0; k < TONE_FREQS; ++k) {      // this lane's entries: {cos, sin} of samples 2l, 2l + 1 and 128 + 2l, 129 + 2l
                    const f4 ta = *(const __attribute__((address_space(1))) f4*)(tg + 2 * (256 * k + 2 * lane));
                    const f4 tb = *(const __attribute__((address_space(1))) f4*)(tg + 2 * (256 * k + 128 + 2 * lane));
                    const float cf = wave_sum_uniform(tone_lane_dot(xq[0][0], xq[0][1], xq[1][0], xq[1][1], ta.x, ta.z, tb.x, tb.z));
                    const float sf = wave_sum_uniform(tone_lane_dot(xq[0][0], xq[0][1], xq[1][0], xq[1][1], ta.y, ta.w, tb.y, tb.w));
                    Pf[k] = tone_power(cf, sf);
                }
                tone_decide(TP, TR, sc(ex), Pf);
                dry = TP.mode == 1.f && TR.guard != 0.f;
                TR.guarded = TR.guarded + TR.guard;
                TR.blocks = TR.blocks + 1.f;
            }
            // the dry gain: 1 at every sample of a guarded block (entering snaps); otherwise g, ramped from the carried p
            const float tg = dry ? 1.f : g;
            const bool ramps = !zs && !dry && gain && ramp && p != g;
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const float ge = ramps ? gain_ramp_at(p, g, 2 * (lane + 64 * q) + e) : tg;
                    mq[q][e] = gain ? wave_mix(ge, xq[q][e], wq[q][e]) : (dry ? xq[q][e] : wq[q][e]);
                    yq[q][e] = zs ? 0.f : mq[q][e];
                }
            if (gain && ramp) p = tg;
            if (alc && !zs) {
                const float ew = wave_sum(alc_lane_sum(wq[0][0], wq[0][1], wq[1][0], wq[1][1]));
                const float pm = wave_max(fmaxf(fmaxf(fabsf(mq[0][0]), fabsf(mq[0][1])), fmaxf(fabsf(mq[1][0]), fabsf(mq[1][1]))));
                float a0, a1;
                alc_decide(P, R, ew, ex, pm, a0, a1);
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int e = 0; e < 2; ++e) yq[q][e] = __fmul_rn(gain_ramp_at(a0, a1, 2 * (lane + 64 * q) + e), mq[q][e]);
            }
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                wave_st(o + 256L * h + 2 * (lane + 64 * q), yq[q][0]);
                wave_st(o + 256L * h + 2 * (lane + 64 * q) + 1, yq[q][1]);
            }
            if (meters) {      // the meters see y; their E_dry is E_x (the same sums in the same order; 0 for a zero block)
                rec.x = __fadd_rn(rec.x, ex);
                rec.y = __fadd_rn(rec.y, wave_sum(alc_lane_sum(yq[0][0], yq[0][1], yq[1][0], yq[1][1])));
                rec.w = __fadd_rn(rec.w, 1.0f);
                pk = fmaxf(pk, fmaxf(fmaxf(fabsf(yq[0][0]), fabsf(yq[0][1])), fmaxf(fabsf(yq[1][0]), fabsf(yq[1][1]))));
            }
            continue;
        }
        bool ramping = false;                      // RAMP: this block mixes with gain_ramp_at(p, g, i)
        if constexpr (RAMP) {
            if (h == 0) {      // (made scalars HERE: in front of the loop the wave would wait for every load issued so far)
                p = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(p)));
                g = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(g)));
                ramping = p != g;
            }
        }
        float ed = 0.f, eo = 0.f;                  // METER: this lane's partial sums of the hop, ((s0^2 + s1^2) + s2^2) + s3^2
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int m = lane + 64 * q;
            const float a0 = prev[q].x + f[q].x, a1 = prev[q].y + f[q].y;
            float g0 = g, g1 = g;      // the dry gains of this lane's two samples: g, but inside a ramping block
            if constexpr (RAMP) {
                if (ramping) {
                    g0 = gain_ramp_at(p, g, 2 * m);
                    g1 = gain_ramp_at(p, g, 2 * m + 1);
                }
            }
            if constexpr (METER) {
                float2 d = dry0[q];
                if (h > 0) {
                    const S* xd = in + (long)n * in_stride + 256L * (h - 1) + 2 * m;
                    d = make_float2(wave_ld(xd), wave_ld(xd + 1));
                }
                const float w0 = ola_div(a0, env[q][0]), w1 = ola_div(a1, env[q][1]);
                // (without gains the plain sample itself: wave_mix(0, x, w) is not w for a non-finite x)
                const float y0 = zero ? 0.f : (gain ? wave_mix(g0, d.x, w0) : w0);
                const float y1 = zero ? 0.f : (gain ? wave_mix(g1, d.y, w1) : w1);
                wave_st(o + 256L * h + 2 * m, y0);
                wave_st(o + 256L * h + 2 * m + 1, y1);
                const float x0 = zero ? 0.f : d.x, x1 = zero ? 0.f : d.y;
                ed = __fadd_rn(q ? __fadd_rn(ed, __fmul_rn(x0, x0)) : __fmul_rn(x0, x0), __fmul_rn(x1, x1));
                eo = __fadd_rn(q ? __fadd_rn(eo, __fmul_rn(y0, y0)) : __fmul_rn(y0, y0), __fmul_rn(y1, y1));
                pk = fmaxf(pk, fmaxf(fabsf(y0), fabsf(y1)));
            } else if constexpr (MIX) {
                float2 d = dry0[q];
                if (h > 0) {
                    const S* xd = in + (long)n * in_stride + 256L * (h - 1) + 2 * m;
                    d = make_float2(wave_ld(xd), wave_ld(xd + 1));
                }
                wave_st(o + 256L * h + 2 * m, zero ? 0.f : wave_mix(g0, d.x, ola_div(a0, env[q][0])));
                wave_st(o + 256L * h + 2 * m + 1, zero ? 0.f : wave_mix(g1, d.y, ola_div(a1, env[q][1])));
            } else {      // (the sample first: the zero then selects between two values, no branch around the division)
                const float w0 = ola_div(a0, env[q][0]), w1 = ola_div(a1, env[q][1]);
                wave_st(o + 256L * h + 2 * m, zero ? 0.f : w0);
                wave_st(o + 256L * h + 2 * m + 1, zero ? 0.f : w1);
            }
            prev[q] = f[q + 2];
        }
        if constexpr (METER) {      // acc = fl(acc + e_h), hop after hop: the record does not depend on how the hops are cut into calls
            rec.x = __fadd_rn(rec.x, wave_sum(ed));
            rec.y = __fadd_rn(rec.y, wave_sum(eo));
            rec.w = __fadd_rn(rec.w, 1.0f);
        }
    }
    if constexpr (METER) {
        rec.z = fmaxf(rec.z, wave_max(pk));
        if (lane == 0) *reinterpret_cast<float4*>(meters + 4 * slot) = rec;
    }
    if constexpr (RAMP) {
        if (lane == 0) ramp[slot] = g;
    }
    if constexpr (ALC) {
        if (meters) rec.z = fmaxf(rec.z, wave_max(pk));      // (wave uniform: every lane takes the shuffles)
        if (lane == 0) {
            if (meters) *reinterpret_cast<float4*>(meters + 4 * slot) = rec;
            if (gain && ramp) ramp[slot] = g;
            if (!none) {
                *reinterpret_cast<float4*>(alc + 8 * slot) = make_float4(R.a, R.S, R.hang, R.voice);
                *reinterpret_cast<float4*>(alc + 8 * slot + 4) = make_float4(R.voiced, R.blocks, 0.f, 0.f);
            }
        }
    }
    if constexpr (GUARD) {
        if (meters) rec.z = fmaxf(rec.z, wave_max(pk));      // (wave uniform: every lane takes the shuffles)
        if (lane == 0) {
            if (meters) *reinterpret_cast<float4*>(meters + 4 * slot) = rec;
            if (gain && ramp) ramp[slot] = p;      // (1 behind a guarded block: the next unguarded one ramps 1 -> g)
            if (!none) {
                if (alc) {
                    *reinterpret_cast<float4*>(alc + 8 * slot) = make_float4(R.a, R.S, R.hang, R.voice);
                    *reinterpret_cast<float4*>(alc + 8 * slot + 4) = make_float4(R.voiced, R.blocks, 0.f, 0.f);
                }
                *reinterpret_cast<float4*>(tone + 8 * slot) = make_float4(TR.tone, TR.cand, TR.run, TR.hold);
                *reinterpret_cast<float4*>(tone + 8 * slot + 4) = make_float4(TR.guard, TR.events, TR.guarded, TR.blocks);
            }
        }
    }
    if constexpr (FLUSH) return;
    // the state: tail = the newest frame's windowed second half; ring = the last 512 input samples; counter (saturating)
#pragma unroll
    for (int q = 0; q < 2; ++q) *reinterpret_cast<float2*>(ws + WS_TAIL + 2 * (lane + 64 * q)) = prev[q];
    const S* xi = in + (long)n * in_stride + 256L * (nhops - 2);     // ring[j] = input sample 256 (nhops - 2) + j
    float2 ring[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = 2 * (lane + 64 * q);
        if (q < 2 && nhops == 1) {      // (this lane's own q + 2; MIX and METER hold the pair already)
            if constexpr (MIX || METER || ALC || GUARD) ring[q] = dry0[q];
            else ring[q] = *reinterpret_cast<const float2*>(ws + WS_RING + 256 + j);
        } else ring[q] = make_float2(wave_ld(xi + j), wave_ld(xi + j + 1));
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<float2*>(ws + WS_RING + 2 * (lane + 64 * q)) = ring[q];
    if (lane == 0) {
        const long c1 = (long)c0 + nhops;
        *reinterpret_cast<int*>(ws + WS_CNT) = c1 > WS_CNT_MAX ? WS_CNT_MAX : (int)c1;
    }
}

// ===================================================================== time spans (offline calls)
// One workgroup per utterance fills the chip only when the batch is a multiple of the 256 CUs: B = 1 (the reference's own
// call shape, infer.py:48) used ONE CU, B = 257 took two rounds.  Every temporal layer of the path is a FIR in time
// (GTConv block: 2 frames of conv history + 2 frames of TRA energies; TCN: 2 d frames), so a kernel's output at frame t
// depends on its input at frames t - H .. t only (H = 12 for the three blocks of the encoder / decoder, 30 for a GTCN
// stack) and the hand-off tensors between the kernels hold ALL frames: each kernel can therefore be cut along time
// independently.  A launch of `nwg` workgroups splits the flattened (utterance, frame) axis into nwg equal shares;
// a share is one or two SEGMENTS (it may run over an utterance boundary); a segment that starts inside an utterance
// is computed from zero history starting H frames early and its first H frames are not stored -- from frame t_lo on
// every value is bit-identical to the unsegmented run (same arithmetic, chunk alignment plays no role:
// chunked == offline holds bit for bit already).  nwg == B gives back one workgroup per utterance, no halo.
// The share of one workgroup is walked segment by segment.  pref (optional, device, int32[B + 1]): prefix sums of the
// utterances' frame counts for a variable-length batch (utterance b holds pref[b+1] - pref[b] <= T frames; T stays the row
// stride of every tensor); nullptr: every utterance has T frames.  Everything here is wave uniform and kept in plain
// 32-bit scalars (structs passed around by reference ended up in scratch memory).
struct SpanIter {
    int g, g1;     // next frame of the flattened (utterance, frame) axis, end of the share
    int b;         // utterance that holds frame g
    int pb;        // flattened index of that utterance's first frame
};
__device__ __forceinline__ bool span_begin(SpanIter& it, int wg, int nwg, int B, int T, const int* __restrict__ pref) {
    const int total = pref ? pref[B] : B * T;
    int per = (total + nwg - 1) / nwg;
    if (pref) per = max(per, 4);             // (uniform batches: the host plan keeps shares above a few frames)
    it.g = wg * per;
    it.g1 = min(total, it.g + per);
    if (it.g >= it.g1) return false;
    if (pref) {
        int lo = 0, hi = B;                  // the utterance with pref[b] <= g < pref[b + 1] (empty ones cannot hold g)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (pref[mid] <= it.g) lo = mid; else hi = mid;
        }
        it.b = lo;
        it.pb = pref[lo];
    } else {
        it.b = it.g / T;
        it.pb = it.b * T;
    }
    return true;
}
// the next segment of the share: utterance sb, first frame processed sfb (halo frames of warm-up in front of the share's
// own first frame, when it starts inside the utterance), first LOCAL frame stored swlo, frames processed snT
__device__ __forceinline__ bool span_next(SpanIter& it, int B, int T, const int* __restrict__ pref, int halo, int& sb, int& sfb,
                                          int& swlo, int& snT) {
    int Tb = 0;
    while (it.g < it.g1) {                   // (skips utterances of zero frames in a prefix table)
        Tb = pref ? pref[it.b + 1] - it.pb : T;
        if (it.g - it.pb < Tb) break;
        it.pb += Tb;
        ++it.b;
    }
    if (it.g >= it.g1) return false;
    const int t_lo = it.g - it.pb, t_hi = min(Tb, it.g1 - it.pb);
    sb = it.b;
    sfb = t_lo > halo ? t_lo - halo : 0;
    swlo = t_lo - sfb;
    snT = t_hi - sfb;
    it.g = it.pb + t_hi;
    return true;
}
constexpr int HALO_BLOCKS = 12;   // three GTConv blocks: 3 x (2 conv frames + 2 TRA energies)
constexpr int HALO_GTCN = 30;     // one GTCN stack: 2 x (1 + 2 + 4 + 8)

// ===================================================================== GTConv block
// GTConvBlock.forward (models/gtcrn_micro.py:229-253) and its streaming twin
// (streaming/gtcrn_micro_stream.py:245-262), in slot space (layout.h / pack.cpp):
//   h  = PReLU(BN(point_conv1(x1)))                     16x16 slot matrix, zero columns on x2 slots
//   hd = PReLU(BN(depth_conv([hist | h])))              encoder: depthwise 3x3 (VALU);
//                                                       decoder: dense transposed 3x3 = 9 slot matrices (MFMA)
//   v  = BN(point_conv2(hd)) written over the x1 slots, x2 slots pass through the C operand
//   TRALite (:122-139): e = mean_F(v^2) per h' channel, causal k=3 conv over [cache | e], 1x1, sigmoid
//   out = v * gate  (gate = 1 on pass-through slots) -- this IS the channel shuffle (:222-227),
//   because the packer renamed the slots instead of moving data.

// per-lane geometry of the wave's TPW tiles; constant for the whole kernel (chunks start at multiples
// of 16 frames, so ring rows -- frame mod 2 / mod 2d -- do not depend on the chunk either)
// (TPW is a template parameter of the model kernels: 3 tiles per wave for full 16-frame chunks, 1 for calls of
// at most SHORT_T frames -- streaming steps -- where the 11 first tiles already cover every valid position)
template <int TPW>
struct Tiles {
    int tl[TPW];    // frame inside the chunk
    int ff[TPW];    // frequency bin
    // position inside the chunk (= tile * 16 + n); one mad, cheaper than a third live register per tile
    __device__ __forceinline__ int pp(int i) const { return __mul24(tl[i], 33) + ff[i]; }
};
template <int TPW, int NWV = NW>
__device__ __forceinline__ Tiles<TPW> make_tiles(const Lane& L) {
    Tiles<TPW> t;
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int p = (L.wave + i * NWV) * 16 + L.n;
        t.tl[i] = p / 33;
        t.ff[i] = p - t.tl[i] * 33;
    }
    return t;
}
// float offset of the lane's record in a 35-column row image (zero pad columns 0 and 34)
constexpr int IMG_R0 = 2;   // image row of the chunk's first frame (rows 0, 1: the two frames before the chunk)
template <int RS, int R0, int PT = 35, int TPW>
__device__ __forceinline__ int o35(const Tiles<TPW>& t, int i, int g) {
    // 24-bit multiplies: full rate (v_mul_lo_u32 is quarter rate and the compiler cannot see the value ranges)
    return __mul24(__mul24(t.tl[i] + R0, PT) + 1 + t.ff[i], RS) + 4 * g;
}

// The spectrogram elements of a chunk a thread handles: item q is element idx = tid + q*NTHR of the chunk,
// idx -> (frame tq, bin f) with f fastest for the frame-major layout and tq fastest for the reference layout
// (consecutive frames adjacent).  One constant division for the first item, increments afterwards.
__device__ __forceinline__ void spec_item_first(int tid, bool t_fast, int& tq, int& f) {
    if (t_fast) { tq = tid & (TC - 1); f = tid >> 4; }
    else { tq = tid / NBINS; f = tid - tq * NBINS; }
}
__device__ __forceinline__ void spec_item_next(bool t_fast, int& tq, int& f) {
    static_assert(NTHR % TC == 0 && NTHR >= 2 * NBINS && NTHR < 3 * NBINS, "item stride decomposition");
    if (t_fast) f += NTHR / TC;
    else {
        f += NTHR - 2 * NBINS;
        tq += 2;
        if (f >= NBINS) { f -= NBINS; ++tq; }
    }
}

struct BlockCtx {
    const float* pb;     // LDS: block parameters (GB_* offsets)
    const float* gA;     // LDS: dense 3x3 slot matrices (decoder) or nullptr
    const int* ib;       // LDS: slot_of_c[8], x2slots[8]
    float* sW;           // LDS: h of this chunk, rows of 35 positions (zero pad columns 0 and 34)
    float* sHk;          // LDS: history ring of h (MS: rows of 35 positions, row = frame & 1; else [2 frames][33][16])
    const float* sHtop;  // not MS: ring to copy into image rows 0, 1 at the top of this block (nullptr: already there)
    const float* sHnext; // not MS: the NEXT block's ring, copied into rows 0, 1 once this block's taps are read (or nullptr)
    float* sS;           // LDS: v^2, [position][16 slots], 33 positions per frame
    float* sG;           // LDS: gates [frame][16 slots]
    float* sEHk;         // LDS: 2-entry ring of e: [frame & 1][8]
    float* sE;           // LDS: energies of the chunk, [2 + TC][8] (rows 0,1: the two frames before it);
                         //      multi-stream mode: [row][3][8] = frames t-2, t-1, t of each row's stream
    float* sY;           // LDS: scratch [rows][8] behind the gate table
    int nfr;             // frames in this chunk (multi-stream mode: live streams of this workgroup)
    int tabs;            // absolute frame index of the chunk's first frame
    // multi-stream mode (MS): image row r holds the ONE new frame of stream r, so every temporal tap comes from that
    // stream's own ring and nothing is shared between rows
    // (per TILE of the wave: the wide single-launch step runs two tiles per wave, whose positions belong to different
    // streams; every other multi-stream form uses entry 0)
    int ms_roff[2];      // per lane: float offset from sW to this block's h ring of the lane's stream
    int ms_tb[2];        // per lane: frame counter of the lane's stream
    const int* sTB;      // LDS: frame counter per row
    // fused single-launch streaming step (k_stream_ms): the h history is a per-block LDS image filled from the stream
    // state; the ONE new row goes straight from the registers to the state (nullptr elsewhere: the rings live in LDS)
    float* g_hist[2];    // per lane: its 16 bytes of the new history row in the stream state, or nullptr
};

// multi-stream geometry of the single-frame streaming step: MS_STREAMS streams per workgroup = rows 0..3 of the
// tile geometry; one tile per wave covers rows 0..5, so the images carry MS_ROWS rows (rows 4, 5 are never stored)
constexpr int MS_STREAMS = 4;
constexpr int MS_ROWS = 6;
constexpr int RING_SET = 3 * 2 * 35 * 16;   // floats of one stream's three 2-row h rings in LDS

// `hook` runs right after the depth-conv phase (register pressure is past its peak there, and two
// barrier intervals of work follow): the decoder uses it to request inputs of later phases early.
// history ring [2 frames][33][16] (older frame first) -> image rows 0, 1 (the pad columns are zeroed per chunk)
template <int RS, int PT = 35, int FMT = IMG_F32>
__device__ __forceinline__ void ring_to_image(float* sW, const float* ring, int tid) {
    if (tid < 2 * 33 * 4) {
        const int row = tid >= 132 ? 1 : 0, r = tid - row * 132;
        const f32x4 v = ld4(ring + (row * 33 + (r >> 2)) * 16 + (r & 3) * 4);
        // (the ring is fp32 whatever the image holds: both conversions are exact)
        if constexpr (FMT == IMG_SPLIT3) st_split(sW, (row * PT + 1 + (r >> 2)) * RS, r & 3, v);
        else if constexpr (FMT == IMG_HALF) st_half(sW, (row * PT + 1 + (r >> 2)) * RS, r & 3, v);
        else st4(sW + pl<RS>(row * PT + 1 + (r >> 2), r & 3), v);
    }
}

// VMK1 >= 0 (dense blocks of the fused streaming step): the DMA of this block's dense planes is waited for at the block's
// FIRST barrier -- `s_waitcnt vmcnt(VMK1)`, VMK1 = the vector-memory operations EVERY wave has issued behind it -- instead
// of at the previous block's closing barrier, which then waits for LDS only.
// NWV: waves of the workgroup (the pair form of the offline encoder runs six); PMAX > 0: the image holds PMAX positions and
// the wave's LAST tile may run past them (its other tiles never do): those lanes compute on whatever they read and store
// nothing into the image
// VMC >= 0: the block's CLOSING barrier also waits for the wave's vector-memory operations down to VMC outstanding
// (the wide streaming step: an LDS-DMA issued a block or more ago becomes visible to every wave there)
template <bool DENSE, int TPW, bool MS, bool Q, int RS, int RSS, bool WIDE_TRA, int PT, int VMK = 0, int VMK1 = -1, int NWV = NW,
          int PMAX = 0, int VMC = -1, class Hook, class Hook3>
__device__ __forceinline__ void gtconv_block(f32x4 (&x)[TPW], const Tiles<TPW>& tin, const BlockCtx& c,
                                             const Lane& L, Hook&& hook, Hook3&& hook3 STAMP_PARAM) {
    static_assert(!MS || TPW <= 2, "multi-stream mode runs one tile per wave (two in the wide single-launch step)");
    // SPLIT: the dense 3x3 on the 16-bit matrix pipe; the image W then holds h as three bf16 planes per position
    constexpr bool SPLIT = DENSE && !Q && kSplitDense;
    constexpr bool HALF = DENSE && Q && !MS;              // the fp16 variant: h as fp16 records, K = 32 chunks
    constexpr int FMT = SPLIT ? IMG_SPLIT3 : (HALF ? IMG_HALF : IMG_F32);
    static_assert(!(SPLIT || HALF) || RS == RS_WIDE, "the split / half image has 96-byte records");
    static_assert(PMAX == 0 || (((!DENSE && !MS) || (MS && !Q)) && NWV * 16 * (TPW - 1) <= PMAX),
                  "partial last tile: depthwise offline form, or the wide single-launch streaming step");
    // (only the wave's LAST tile can run past PMAX)
    auto in_image = [&](int i) -> bool { return PMAX == 0 || i < TPW - 1 || tin.pp(i) < PMAX; };
    constexpr int NT = NWV * 64;
    const int n = L.n, g = L.g;
    // Image rows (not MS): rows 0, 1 hold the two frames BEFORE the chunk -- copied from the block's history ring at
    // the top of the block -- and row 2 + tl holds frame tl of the chunk, so a temporal tap is always "own record minus
    // a constant": no per-lane choice between image and ring, no select, no second address (IMG_R0 = 2).
    // MS: row r holds the one new frame of stream r and the taps come from that stream's own parity-indexed ring.
    constexpr int R0 = MS ? 0 : IMG_R0;
    // (The offsets are derived from an opaque copy of the tiles' rows: recomputed per block -- a few full-rate integer
    // ops -- instead of being hoisted out of the chunk loop and held in registers across the whole kernel.)
    Tiles<TPW> tt = tin;
#pragma unroll
    for (int i = 0; i < TPW; ++i) asm volatile("" : "+v"(tt.tl[i]));
    int b0s[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) b0s[i] = o35<RS, R0, PT>(tt, i, g);
    // float offset (from sW) of the record `back` frames before tile i's own position b0
    auto tap_base = [&](int i, int back, int b0) -> int {
        if constexpr (MS) return back == 0 ? b0 : c.ms_roff[i] + (((c.ms_tb[i] + back) & 1) * 35 + 1 + tt.ff[i]) * RS + 4 * g;
        else return b0 - back * PT * RS;
    };
    if constexpr (!MS) {
        if (c.sHtop) ring_to_image<RS, PT, FMT>(c.sW, c.sHtop, L.tid);
    }
    const float a1 = slope_arg<Q>(c.pb[GB_SLOPE]), a2 = slope_arg<Q>(c.pb[GB_SLOPE + 1]);
    // ---- point_conv1 + BN + PReLU; h lives only in the LDS image from here on (its centre tap and the
    //      ring update re-read it: one ds_read_b128 each instead of 12 registers held across the phase) ----
    {
        f32x4 h[TPW];
        const f32x4 A = ld4(c.pb + GB_PC1_A + arow(n, g)), Bv = ld4(c.pb + GB_PC1_B + 4 * g);
#pragma unroll
        for (int i = 0; i < TPW; ++i) h[i] = Bv;
        mm16<TPW, Q>(A, x, h);
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const f32x4 hv = rq<Q>(prelu4q<Q>(h[i], a1));
            if constexpr (SPLIT) { if (in_image(i)) st_split(c.sW, b0s[i] - 4 * g, g, hv); }
            else if constexpr (HALF) st_half(c.sW, b0s[i] - 4 * g, g, hv);
            else if (in_image(i)) st4(c.sW + b0s[i], hv);
            if constexpr (MS) {
                if (c.g_hist[i] && tt.tl[i] < c.nfr) st4(c.g_hist[i], hv);     // the stream's new history row (replaces frame t-2)
            }
        }
    }
    // Fused streaming step, dense blocks: this block's dense planes were requested by LDS-DMA behind the PREVIOUS block's
    // dense phase and are first read behind this barrier.  Vector-memory operations a wave has issued since: the two
    // history loads of the next block (every wave issues both) and the new-row store above (live lanes only: not every
    // wave) -- so "at most two outstanding" (VMK1 = 2) retires the DMA in every wave.
    if constexpr (VMK1 >= 0) wg_barrier_vm<VMK1>();
    else wg_barrier();
    STAMP(SS, 5)
    // ---- depth conv + BN + PReLU, then point_conv2 + BN in place over the x1 slots; one tile at a
    //      time so that the tap registers die with the tile (the partner waves on the SIMD fill the
    //      MFMA dependency gaps); v^2 is reduced over the tile's 16 positions in registers -----------
    {
        const f32x4 Bd = ld4(c.pb + GB_DW_B + 4 * g);
        const f32x4 A2 = ld4(c.pb + GB_PC2_A + arow(n, g)), B2 = ld4(c.pb + GB_PC2_B + 4 * g);
        const f32x4 keep = ld4(c.pb + GB_KEEP + 4 * g);
        if constexpr (!DENSE) {
            // depthwise 3x3, kernel-row major: the three weights of a kernel row stay in registers for all of the
            // wave's tiles (9 LDS weight reads per block instead of 9 per tile; this phase is LDS-bound)
            f32x4 acc[TPW];
#pragma unroll
            for (int i = 0; i < TPW; ++i) acc[i] = Bd;
#pragma unroll
            for (int kt = 0; kt < 3; ++kt) {
                const f32x4 w0 = ld4(c.pb + GB_DW_W + (kt * 3 + 0) * 16 + 4 * g);
                const f32x4 w1 = ld4(c.pb + GB_DW_W + (kt * 3 + 1) * 16 + 4 * g);
                const f32x4 w2 = ld4(c.pb + GB_DW_W + (kt * 3 + 2) * 16 + 4 * g);
                const int back = 2 - kt;                     // tap (t-2+kt, f-1+kf)
#pragma unroll
                for (int i = 0; i < TPW; ++i) {
                    const int b0 = b0s[i];
                    const int rb = tap_base(i, back, b0);
                    // three fused multiply-adds per component (a sum of products added afterwards costs a fourth op)
                    // (the side taps from the centre record by DPP row shifts -- 9 instead of 27 reads per wave and block --
                    // measured SLOWER even without the edge lanes' extra reads: profiles/r06_ab_encoder_dpp.txt)
                    acc[i] += w0 * ld4(c.sW + rb - RS);
                    acc[i] += w1 * ld4(c.sW + rb);
                    acc[i] += w2 * ld4(c.sW + rb + RS);
                }
            }
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                acc[i] = rq<Q>(prelu4q<Q>(acc[i], a2));
                x[i] = keep * x[i] + B2;
            }
            mm16<TPW, Q>(A2, acc, x);                         // point_conv2: the tiles' chains interleaved
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                x[i] = rq<Q>(x[i]);
                if (!MS || in_image(i)) st4(c.sS + tt.pp(i) * RSS + 4 * g, x[i] * x[i]);   // energies are reduced cooperatively after the barrier
            }
        } else if constexpr (SPLIT) {
            // dense transposed 3x3 on v_mfma_f32_16x16x32_bf16: K-chunk cc = taps 2cc and 2cc+1 (k = tap half * 16 + hidden
            // channel; the lane groups g < 2 hold the first tap, g >= 2 the second); per chunk the three weight planes are
            // read once per wave, the three h planes once per tile, six products per tile (small ones first)
            f32x4 acc[TPW];
            int rec0[TPW];
#pragma unroll
            for (int i = 0; i < TPW; ++i) { acc[i] = Bd; rec0[i] = b0s[i] - 4 * g; }
            // (from an opaque copy of g: the five per-chunk tap selects are recomputed per block -- five vector ops --
            // instead of being hoisted out of the chunk loop and spilled)
            int gq = g;
            asm volatile("" : "+v"(gq));
            const bool second = gq >= 2;
            const int q16 = 4 * (gq & 1);                    // channels 0..7 / 8..15 of the plane
            // float offset of the record `back` frames before tile i's own one (MS: in that stream's ring)
            auto rec_back = [&](int i, int back) -> int {
                if constexpr (MS) return back == 0 ? rec0[i] : c.ms_roff[i] + (((c.ms_tb[i] + back) & 1) * 35 + 1 + tt.ff[i]) * RS;
                else return rec0[i] - back * PT * RS;
            };
#pragma unroll
            for (int cc = 0; cc < DN16_CHUNKS; ++cc) {
                constexpr int NT = 9;
                // chunk 4 has one tap: the lane groups g >= 2 meet zero weights and read some valid record -- the one of
                // tap 7, an ODD number of records away from tap 8's: lanes (n, g) and (n, g + 2) then fall 8 banks apart
                // like the slot groups of an fp32 record, and the tile-wide ds_read_b128 stays conflict free (the other
                // four chunks pair taps that are an odd number of records apart by themselves)
                // (same-box A/B against tap 8: 0.4060 vs 0.4051 ms -- inside the noise; kept for the cleaner pattern)
                const int tA = 2 * cc, tB = 2 * cc + 1 < NT ? 2 * cc + 1 : NT - 2;
                bf16x8 ap[3];
#pragma unroll
                for (int p = 0; p < 3; ++p) ap[p] = *reinterpret_cast<const bf16x8*>(c.gA + (cc * 3 + p) * 256 + arow(n, g));
#pragma unroll
                for (int i = 0; i < TPW; ++i) {
                    // decoder (transposed): tap (kt, kf) reads (t - kt, f + 1 - kf)
                    const int ra = rec_back(i, tA / 3) + (1 - tA % 3) * RS, rb = rec_back(i, tB / 3) + (1 - tB % 3) * RS;
                    const float* src = c.sW + (second ? rb : ra) + q16;
                    bf16x8 bp[3];
#pragma unroll
                    for (int p = 0; p < 3; ++p) bp[p] = *reinterpret_cast<const bf16x8*>(src + 8 * p);
                    acc[i] = split_mm6(ap, bp, acc[i]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                acc[i] = prelu4(acc[i], a2);
                x[i] = keep * x[i] + B2;
            }
            mm16<TPW, Q>(A2, acc, x);                         // point_conv2: the tiles' chains interleaved
#pragma unroll
            for (int i = 0; i < TPW; ++i)
                if (!MS || in_image(i)) st4(c.sS + tt.pp(i) * RSS + 4 * g, x[i] * x[i]);
        } else if constexpr (HALF) {
            // the fp16 variant: same K-chunks, one plane: per chunk one weight read per wave, one h read and ONE
            // v_mfma_f32_16x16x32_f16 per tile
            f32x4 acc[TPW];
            int rec0[TPW];
#pragma unroll
            for (int i = 0; i < TPW; ++i) { acc[i] = Bd; rec0[i] = b0s[i] - 4 * g; }
            int gq = g;
            asm volatile("" : "+v"(gq));
            const bool second = gq >= 2;
            const int q16 = 4 * (gq & 1);
#pragma unroll
            for (int cc = 0; cc < DN16_CHUNKS; ++cc) {
                const int tA = 2 * cc, tB = 2 * cc + 1 < 9 ? 2 * cc + 1 : 7;   // (chunk 4: see the split form)
                const h16x8 ap = *reinterpret_cast<const h16x8*>(c.gA + cc * 256 + arow(n, g));
#pragma unroll
                for (int i = 0; i < TPW; ++i) {
                    const int ra = rec0[i] - (tA / 3) * PT * RS + (1 - tA % 3) * RS, rb = rec0[i] - (tB / 3) * PT * RS + (1 - tB % 3) * RS;
                    const h16x8 bp = *reinterpret_cast<const h16x8*>(c.sW + (second ? rb : ra) + q16);
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ap, bp, acc[i], 0, 0, 0);
                }
            }
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                acc[i] = rq<Q>(prelu4q<Q>(acc[i], a2));
                x[i] = keep * x[i] + B2;
            }
            mm16<TPW, Q>(A2, acc, x);
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                x[i] = rq<Q>(x[i]);
                st4(c.sS + tt.pp(i) * RSS + 4 * g, x[i] * x[i]);
            }
        } else {
            // dense transposed 3x3, tap major: each of the nine 16x16 slot matrices is read from LDS once per wave
            // (not once per tile) and feeds one MFMA chain per tile -- TPW independent accumulator chains
            f32x4 acc[TPW];
#pragma unroll
            for (int i = 0; i < TPW; ++i) acc[i] = Bd;
#pragma unroll
            for (int kt = 0; kt < 3; ++kt) {
#pragma unroll
                for (int kf = 0; kf < 3; ++kf) {
                    const f32x4 A = ld4(c.gA + (kt * 3 + kf) * 256 + arow(n, g));
                    const int back = kt, df = 1 - kf;        // decoder (transposed): tap (t-kt, f+1-kf)
#pragma unroll
                    for (int i = 0; i < TPW; ++i) {
                        const int b0 = b0s[i];
                        const int rb = tap_base(i, back, b0);
                        const f32x4 tap = ld4(c.sW + rb + df * RS);
                        acc[i] = mm1<Q>(A, tap, acc[i]);
                    }
                    // one tap's loads (a matrix + TPW records) in flight at a time: hoisting more of them ahead of
                    // the MFMAs pushes the kernel into scratch
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                acc[i] = rq<Q>(prelu4q<Q>(acc[i], a2));
                x[i] = keep * x[i] + B2;
            }
            mm16<TPW, Q>(A2, acc, x);                         // point_conv2: the tiles' chains interleaved
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                x[i] = rq<Q>(x[i]);
                st4(c.sS + tt.pp(i) * RSS + 4 * g, x[i] * x[i]);   // energies are reduced cooperatively after the barrier
            }
        }
    }
    wg_barrier();
    STAMP(SS, 6)
    // (single-frame steps: hook3 -- the next block's history image, whose loads were requested a block ago -- runs FIRST:
    // the waits the compiler puts in front of those registers also drain every vector-memory operation issued before
    // them, and hook() is where the next block's dense planes go out by DMA)
    if constexpr (MS) hook3();
    hook();
    // ---- history ring of h (after every wave has read its taps): the last two frames of the image ---------------
    if constexpr (MS) {
        // (same record format in the image and in the LDS ring: a copy of the lane's 16 bytes -- SPLIT: three planes'
        // 8 bytes, which sit at float offsets 2g, 8 + 2g, 16 + 2g of the 96-byte record)
#pragma unroll
        for (int i = 0; i < TPW; ++i)
            if (tt.tl[i] < c.nfr && !c.g_hist[i]) {
                const int dst = c.ms_roff[i] + ((c.ms_tb[i] & 1) * 35 + 1 + tt.ff[i]) * RS;
                if constexpr (SPLIT) {
#pragma unroll
                    for (int p = 0; p < 3; ++p)
                        *reinterpret_cast<f32x2*>(c.sW + dst + 8 * p + 2 * g) =
                            *reinterpret_cast<const f32x2*>(c.sW + b0s[i] - 4 * g + 8 * p + 2 * g);
                } else {
                    st4(c.sW + dst + 4 * g, ld4(c.sW + b0s[i]));
                }
            }
    } else {
        // frames nfr-2, nfr-1 of the chunk = image rows nfr, nfr+1 (for a one-frame call row nfr is the old row 1)
        if (L.tid >= NT - 2 * 33 * 4) {
            const int q = L.tid - (NT - 2 * 33 * 4), row = q >= 132 ? 1 : 0, r = q - row * 132;
            float* dst = c.sHk + (row * 33 + (r >> 2)) * 16 + (r & 3) * 4;
            if constexpr (SPLIT) st4(dst, ld_split(c.sW, ((c.nfr + row) * PT + 1 + (r >> 2)) * RS, r & 3));   // exact
            else if constexpr (HALF) st4(dst, ld_half(c.sW, ((c.nfr + row) * PT + 1 + (r >> 2)) * RS, r & 3));
            else st4(dst, ld4(c.sW + pl<RS>((c.nfr + row) * PT + 1 + (r >> 2), r & 3)));
        }
    }
    if constexpr (MS) {
        // ---- TRALite of a single-frame step, ONE barrier interval.  Every image row is its own stream with ONE new
        //      frame, so the energies of frames t-2, t-1 come from that stream's ring (sEHk), not from other threads: the
        //      lane that holds a channel's total (part == 0 of its DPP quad) goes straight on to the causal conv1d, the
        //      1x1 and the sigmoid -- the eight channels of a frame sit in one wave and meet through wave-private LDS.
        //      Same sums in the same order, same expressions as the two-step form below: bit-identical gates.  (The
        //      next block's history image -- hook3 -- has only to wait for this block's taps: it ran above.)
        int tz1 = L.tid;
        asm volatile("" : "+v"(tz1));
        const int part = tz1 & 3, rc = (tz1 >> 2) & 7, rt = tz1 >> 5;
        if (tz1 < c.nfr * 32) {
            float sum = 0.f;
            {
                const float* sp = c.sS + (rt * 33 + (part == 3 ? 24 : part * 9)) * RSS + c.ib[rc];
                float v[9];
#pragma unroll
                for (int f = 0; f < 9; ++f) v[f] = sp[f * RSS];
#pragma unroll
                for (int f = 0; f < 9; ++f) sum += (f < 3 && part == 3) ? 0.f : v[f];
            }
            // the ring entries and this channel's parameters: requested beside the energy loads
            const int tb = c.sTB[rt];
            const float e2 = c.sEHk[rt * 48 + ((tb - 2) & 1) * 8 + rc], e1 = c.sEHk[rt * 48 + ((tb - 1) & 1) * 8 + rc];
            sum += dpp_ror<0xB1>(sum);   // quad_perm [1,0,3,2]
            sum += dpp_ror<0x4E>(sum);   // quad_perm [2,3,0,1]
            if (part == 0) {
                const int ro = rc;
                const float e0 = sum * (1.0f / 33.0f);
                const float y = c.pb[GB_TRA_DB + ro] + c.pb[GB_TRA_DW + ro * 3] * e2 +
                                c.pb[GB_TRA_DW + ro * 3 + 1] * e1 + c.pb[GB_TRA_DW + ro * 3 + 2] * e0;
                float* sy = c.sY + rt * 8;
                sy[ro] = y;
                wave_lds_sync();
                float z = c.pb[GB_TRA_PB + ro];
#pragma unroll
                for (int cc = 0; cc < 8; ++cc) z += c.pb[GB_TRA_PW + ro * 8 + cc] * sy[cc];
                c.sG[rt * 16 + c.ib[ro]] = rq1<Q>(__frcp_rn(1.0f + __expf(-z)));
                c.sG[rt * 16 + c.ib[8 + ro]] = 1.0f;
                c.sEHk[rt * 48 + (tb & 1) * 8 + ro] = e0;        // the new frame's energy replaces frame t-2's
            }
        }
    } else {
        // ---- TRALite, step 1: energies e[t][c] = mean_F(v^2): 32 threads per frame = 8 h' channels x 4 bin
        //      ranges (9, 9, 9, 6 bins); the four partial sums of a channel sit in one DPP quad and are
        //      combined there in a fixed order (bit-reproducible).  Written to sE[2 + t][c]; rows 0,1 of sE
        //      hold the two frames before the chunk (the block's energy ring) ---------------------------------
        {
            // (index arithmetic from an opaque copy of tid: recomputed per block instead of hoisted out of the block and
            // chunk loops, kept live across the whole kernel and spilled -- a scratch reload drains every load in flight)
            int tz1 = L.tid;
            asm volatile("" : "+v"(tz1));
            const int part = tz1 & 3, rc = (tz1 >> 2) & 7, rt = tz1 >> 5;
            if (tz1 < c.nfr * 32) {
                // nine independent loads per thread (the last range, bins 27..32, reads bins 24..32 and drops the first
                // three), then the same ascending-bin summation as a 9 / 6-trip loop -- whose loads went out one by one
                float sum = 0.f;
                if constexpr (WIDE_TRA) {
                    const float* sp = c.sS + (rt * 33 + (part == 3 ? 24 : part * 9)) * RSS + c.ib[rc];
                    float v[9];
    #pragma unroll
                    for (int f = 0; f < 9; ++f) v[f] = sp[f * RSS];
    #pragma unroll
                    for (int f = 0; f < 9; ++f) sum += (f < 3 && part == 3) ? 0.f : v[f];
                } else {   // (the one instantiation with no registers to spare: the same sums from a loop)
                    const float* sp = c.sS + (rt * 33 + part * 9) * RSS + c.ib[rc];
                    const int cnt = part == 3 ? 6 : 9;
                    for (int f = 0; f < cnt; ++f) sum += sp[f * RSS];
                }
                sum += dpp_ror<0xB1>(sum);   // quad_perm [1,0,3,2]
                sum += dpp_ror<0x4E>(sum);   // quad_perm [2,3,0,1]
                if (part == 0) c.sE[(MS ? rt * 3 + 2 : 2 + rt) * 8 + rc] = sum * (1.0f / 33.0f);
            } else if (MS && tz1 >= NT - 64) {    // an otherwise idle wave copies every stream's ring into its rows 0,1
                const int q = tz1 - (NT - 64), sidx = q >> 4, r = (q >> 3) & 1, cc = q & 7;
                if (sidx < c.nfr) c.sE[(sidx * 3 + r) * 8 + cc] = c.sEHk[sidx * 48 + ((c.sTB[sidx] - 2 + r) & 1) * 8 + cc];
            } else if (!MS && tz1 >= NT - 16) {   // an otherwise idle wave copies the ring into rows 0,1
                const int q = tz1 - (NT - 16), r = q >> 3, cc = q & 7;
                c.sE[r * 8 + cc] = c.sEHk[((c.tabs - 2 + r) & 1) * 8 + cc];
            }
        }
        wg_barrier();
        // rows 0, 1 of the image are free (this block's ring save, which may read row 1, is behind the barrier): the next
        // block's history goes there now, off the critical path
        if constexpr (!MS) {
            if (c.sHnext) ring_to_image<RS, PT, FMT>(c.sW, c.sHnext, L.tid);
        }
        hook3();   // (k_stream_ms: the next block's history image, its taps are all read)
        // ---- step 2: one thread per (frame, output channel): causal depthwise conv1d (k=3) over the energies,
        //      1x1 conv, sigmoid (models/gtcrn_micro.py:122-139) ------------------------------------------------
        {
            int tz2 = L.tid;
            asm volatile("" : "+v"(tz2));
            const int ro = tz2 & 7, rt = tz2 >> 3;
            if (tz2 < c.nfr * 8) {
                const float* e = c.sE + (MS ? rt * 24 : rt * 8) + ro;    // rows rt, rt+1, rt+2 = frames t-2, t-1, t
                const float y = c.pb[GB_TRA_DB + ro] + c.pb[GB_TRA_DW + ro * 3] * e[0] +
                                c.pb[GB_TRA_DW + ro * 3 + 1] * e[8] + c.pb[GB_TRA_DW + ro * 3 + 2] * e[16];
                // the 8 channels of a frame sit in 8 adjacent lanes of one wave: exchange y through the
                // scratch behind the gate table with wave-local ordering, no workgroup barrier
                float* sy = c.sY + rt * 8;
                sy[ro] = y;
                wave_lds_sync();
                float z = c.pb[GB_TRA_PB + ro];
    #pragma unroll
                for (int cc = 0; cc < 8; ++cc) z += c.pb[GB_TRA_PW + ro * 8 + cc] * sy[cc];
                c.sG[rt * 16 + c.ib[ro]] = rq1<Q>(__frcp_rn(1.0f + __expf(-z)));
                c.sG[rt * 16 + c.ib[8 + ro]] = 1.0f;
                // the last two frames' energies become the ring for the next chunk (row = frame & 1)
                if constexpr (MS) c.sEHk[rt * 48 + (c.sTB[rt] & 1) * 8 + ro] = e[16];
                else if (rt >= c.nfr - 2) c.sEHk[((c.tabs + rt) & 1) * 8 + ro] = e[16];
            }
        }
    }
    // the decoder's hook started the next block's weight DMA two barriers ago; the VMK loads it issued behind the DMA
    // (en_outs[0] for the tail) stay in flight
    if constexpr (VMC >= 0) wg_barrier_vm<VMC>();
    else if constexpr (DENSE && VMK1 < 0) wg_barrier_vm<VMK>();
    else wg_barrier();               // (VMK1 >= 0: the DMA is waited for at the next block's first barrier)
    STAMP(SS, 7)
#pragma unroll
    for (int i = 0; i < TPW; ++i) x[i] = rq<Q>(x[i] * ld4(c.sG + tt.tl[i] * 16 + 4 * g));
}

// zero the two pad columns of the TC rows of a 35-position row image (tid and the zero are made
// opaque so that neither is hoisted out of the chunk loop and kept live / spilled)
template <int ROWS = TC, int RS = 16, int PT = 35>
__device__ __forceinline__ void zero_row_pads(float* img, int tid) {
    asm volatile("" : "+v"(tid));
    // all RS floats of the record: a split image (three bf16 planes) uses the full 96 bytes
    static_assert(ROWS * 2 * 8 <= NTHR && RS <= 32, "one thread per 16-byte piece");
    if (tid < ROWS * 2 * 8) {
        const int r = tid >> 4, side = (tid >> 3) & 1, gg = tid & 7;
        float z = 0.f;
        asm volatile("" : "+v"(z));
        if (gg < RS / 4) st4(img + (r * PT + side * 34) * RS + 4 * gg, splat(z));
    }
}

// load / store the h rings and e rings of 3 blocks from / to the stream state.  LDS: [3 blocks][2 frames][33][16],
// the OLDER frame first (gtconv_block copies it into image rows 0, 1); state: row = frame & 1 (the layout the
// multi-stream form reads in place), so frame tb - 2 + r of a stream whose next frame is tb sits in state row (tb + r) & 1.
constexpr int RING_DENSE = 2 * 33 * 16;     // floats of one block's ring in LDS (single-stream kernels)
__device__ __forceinline__ void rings_load(float* sH, float* sEH, const float* st_h, const float* st_e, int tb, int tid) {
    for (int i = tid; i < 3 * 2 * 33 * 4; i += NTHR) {
        const int gg = i & 3, pos = i >> 2;           // pos over 3 blocks x 2 frames x 33 bins
        const int f = pos % 33, br = pos / 33, r = br & 1;
        f32x4 v = splat(0.f);
        if (st_h) v = ld4(st_h + ((br - r + ((tb + r) & 1)) * 33 + f) * 16 + gg * 4);
        st4(sH + pos * 16 + gg * 4, v);
    }
    if (tid < 48) sEH[tid] = st_e ? st_e[tid] : 0.f;
}
// The same for the NS streams of a multi-stream workgroup in ONE pass: all of a thread's loads are issued before its
// first store (four back-to-back single-stream passes would expose four global-load latencies in the prologue of a
// kernel whose whole run time is a few of them).  st0 = state of the workgroup's first stream, h_off / e_off = float
// offsets of the ring sets inside a stream's state; streams >= nlive get zero rings.
// RS = 16: fp32 records; RS = 24 (SPLIT, the decoder): the three-plane bf16 records the dense 3x3 reads (the state in
// HBM holds fp32 either way: the split is exact, so is its inverse in rings_store_ms).
template <int NS, int RS = 16>
__device__ __forceinline__ void rings_load_ms(float* sH, float* sEH, const float* st0, int h_off, int e_off, int nlive,
                                              int tid) {
    constexpr bool SPLIT = RS == RS_WIDE;
    constexpr int RSET = 3 * 2 * 35 * RS;
    constexpr int PER = 3 * 2 * 35 * 4;                        // float4 items of one stream's image (pad columns included)
    constexpr int ITEMS = (NS * PER + NTHR - 1) / NTHR;
    f32x4 v[ITEMS];
#pragma unroll
    for (int q = 0; q < ITEMS; ++q) {
        const int i = tid + q * NTHR;
        const int sidx = i / PER, r = i - sidx * PER, gg = r & 3, pos = r >> 2, col = pos % 35, br = pos / 35;
        v[q] = splat(0.f);
        if (i < NS * PER && sidx < nlive && col >= 1 && col <= 33)
            v[q] = ld4(st0 + (long)sidx * ST_FLOATS + h_off + ((br * 33) + col - 1) * 16 + gg * 4);
    }
#pragma unroll
    for (int q = 0; q < ITEMS; ++q) {
        const int i = tid + q * NTHR;
        const int sidx = i / PER, r = i - sidx * PER;
        if (i < NS * PER) {
            if constexpr (SPLIT) st_split(sH, sidx * RSET + (r >> 2) * RS, r & 3, v[q]);
            else st4(sH + sidx * RSET + pl(r >> 2, r & 3), v[q]);
        }
    }
    if (tid < NS * 48) {
        const int sidx = tid / 48, e = tid - sidx * 48;
        sEH[tid] = sidx < nlive ? st0[(long)sidx * ST_FLOATS + e_off + e] : 0.f;
    }
}
template <int NS, int RS = 16>
__device__ __forceinline__ void rings_store_ms(const float* sH, const float* sEH, float* st0, int h_off, int e_off,
                                               int nlive, int tid) {
    constexpr bool SPLIT = RS == RS_WIDE;
    constexpr int RSET = 3 * 2 * 35 * RS;
    constexpr int PER = 3 * 2 * 33 * 4;
    for (int i = tid; i < nlive * PER; i += NTHR) {
        const int sidx = i / PER, r = i - sidx * PER, gg = r & 3, pos = r >> 2, f = pos % 33, br = pos / 33;
        f32x4 v;
        if constexpr (SPLIT) v = ld_split(sH, sidx * RSET + (br * 35 + 1 + f) * RS, gg);
        else v = ld4(sH + sidx * RSET + pl(br * 35 + 1 + f, gg));
        st4(st0 + (long)sidx * ST_FLOATS + h_off + pos * 16 + gg * 4, v);
    }
    if (tid < nlive * 48) {
        const int sidx = tid / 48, e = tid - sidx * 48;
        st0[(long)sidx * ST_FLOATS + e_off + e] = sEH[tid];
    }
}
// tb = the stream's NEXT frame index after this call (the LDS rings hold frames tb - 2, tb - 1)
__device__ __forceinline__ void rings_store(const float* sH, const float* sEH, float* st_h, float* st_e, int tb, int tid) {
    for (int i = tid; i < 3 * 2 * 33 * 4; i += NTHR) {
        const int gg = i & 3, pos = i >> 2;
        const int f = pos % 33, br = pos / 33, r = br & 1;
        st4(st_h + ((br - r + ((tb + r) & 1)) * 33 + f) * 16 + gg * 4, ld4(sH + pos * 16 + gg * 4));
    }
    if (tid < 48) st_e[tid] = sEH[tid];
}

// Store a tile in the slot order of its consumer.  The permutation crosses lane groups, so it goes
// through LDS: each lane scatters its 4 slots into the position's 64-byte record of a wave-private
// scratch image (LDS handles 4-byte scatters at full rate), reads the record back as its own 16-byte
// quarter and issues ONE coalesced 16-byte global store.  (Scattering 4-byte global stores instead
// writes 64 partial lines per instruction and was ~3 k cycles per block.)  The four lanes of a
// position belong to one wave, LDS operations of a wave complete in order, so no barrier is needed.
// Scratch records PERM_RS = 20 floats apart: the 4-byte scatters of 32 lanes (16 positions x 2 slot groups) then spread
// over the banks (2-way); at the 16-float pitch of a dense record image they pile up on four banks (8-way).
constexpr int PERM_RS = 20;
__device__ __forceinline__ f32x4 permute_via_lds(float* scratch_rec, const int* idx4, int g, f32x4 v) {
    scratch_rec[idx4[0]] = v[0];
    scratch_rec[idx4[1]] = v[1];
    scratch_rec[idx4[2]] = v[2];
    scratch_rec[idx4[3]] = v[3];
    wave_lds_sync();
    return ld4(scratch_rec + 4 * g);
}

// The inverse: a record held in its consumer's slot order -> this lane's own slots (the same index table).
__device__ __forceinline__ f32x4 unpermute_via_lds(float* scratch_rec, const int* idx4, int g, f32x4 y) {
    st4(scratch_rec + 4 * g, y);
    wave_lds_sync();
    f32x4 v = {scratch_rec[idx4[0]], scratch_rec[idx4[1]], scratch_rec[idx4[2]], scratch_rec[idx4[3]]};
    return v;
}

// The same for all of a wave's tiles at once: the index table is read once, all scatters (or record writes) go out
// together and ONE wave-local sync separates them from the reads -- three LDS round trips per call instead of three
// per tile (these sit in short barrier-delimited phases whose length is their longest dependency chain).
template <int N>
__device__ __forceinline__ void permute_tiles_via_lds(float* scratch, const int (&off)[N], const int* idx4, int g,
                                                      const f32x4 (&v)[N], f32x4 (&y)[N]) {
    const int i0 = idx4[0], i1 = idx4[1], i2 = idx4[2], i3 = idx4[3];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        float* r = scratch + off[i];
        r[i0] = v[i][0]; r[i1] = v[i][1]; r[i2] = v[i][2]; r[i3] = v[i][3];
    }
    wave_lds_sync();
#pragma unroll
    for (int i = 0; i < N; ++i) y[i] = ld4(scratch + off[i] + 4 * g);
}
template <int N>
__device__ __forceinline__ void unpermute_tiles_via_lds(float* scratch, const int (&off)[N], const int* idx4, int g,
                                                        const f32x4 (&y)[N], f32x4 (&v)[N]) {
    const int i0 = idx4[0], i1 = idx4[1], i2 = idx4[2], i3 = idx4[3];
#pragma unroll
    for (int i = 0; i < N; ++i) st4(scratch + off[i] + 4 * g, y[i]);
    wave_lds_sync();
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float* r = scratch + off[i];
        v[i][0] = r[i0]; v[i][1] = r[i1]; v[i][2] = r[i2]; v[i][3] = r[i3];
    }
}

// =============================================================================== encoder
// spec -> [mag,re,im] (models/gtcrn_micro.py:510-515) -> ERB.bm (:63-67) -> SFE_Lite (:77-90)
// -> en_convs.0/1 (ConvBlock :142-164, Conv2d (1,5) stride (1,2)) -> 3 x GTConvBlock (:365-393).
// Writes the five skip tensors en0 (B,T,65,16) and en1..en4 (B,T,33,16); en1..en3 are written in
// the slot order of the decoder stage that consumes them (layout.h I_ENST), en4 in its own order.
// LDS carve of k_encoder: RW image rows (TC, or MS_ROWS in multi-stream mode), NS ring sets (streams per workgroup)
constexpr int ENC_E0_ROW = 69;
constexpr int ENC_I_SKIP = I_ENC_BLK - I_BS_LO;   // integer tables the encoder never reads (not copied to LDS)
static_assert(I_BS_LO == 128 && I_BS_N + 192 == I_ENC_BLK && ENC_I_SKIP % 4 == 0, "integer table layout");
constexpr int EB_ROW = 131, F0_ROW = 136;
template <int RW, int NS, bool MS, bool FRONT>
struct EncLds {
    static constexpr int RS = FRONT ? 16 : RS_WIDE;            // record pitch of the block images W, S and the h rings
    static constexpr int P = 0;
    static constexpr int I = P + ENC_SIZE;
    static constexpr int H = I + P_INTS - ENC_I_SKIP;
    static constexpr int EH = H + (MS ? NS * RING_SET : 3 * RING_DENSE);
    static constexpr int TB = EH + NS * 48;                    // frame counter per row (ints; multi-stream mode)
    static constexpr int G = TB + 8;
    static constexpr int E = G + RW * 16 + RW * 8;             // (gates [RW][16] + y scratch [RW][8]); energies
    static constexpr int A = E + (MS ? NS * 24 : (RW + 2) * 8);   // FRONT: staged spec, then E0, then W + S; else W
    static constexpr int RWI = MS ? RW : RW + IMG_R0;         // image rows (two history rows in front of the chunk)
    // image row pitch in records: 35 = 33 bins + two zero pad columns.  The offline form has LDS to spare and uses 41:
    // a 16-position tile that runs over the end of a row then continues 9 = 1 (mod 8) records further on, so the
    // conflict-free bank pattern of the 96-byte records (pl()) also holds for the ~half of the tiles that wrap (-2.6 %)
    static constexpr int PT = FRONT ? 35 : 41;
    static constexpr int B = A + (FRONT ? RW * ENC_E0_ROW * 16 : RWI * PT * RS);   // FRONT: EB + F0; else S
    static constexpr int S = FRONT ? A + RWI * 35 * 16 : B;   // FRONT: S may run over into B (EB / F0 are dead by then)
    static constexpr int FLOATS = B + (FRONT ? 3 * RW * EB_ROW + 3 * RW * F0_ROW : RW * 33 * RS);
    static_assert(3 * RW * NBINS <= RW * ENC_E0_ROW * 16, "staged [mag,re,im] chunk must fit in the E0 region");
    static_assert(FLOATS * 4 <= 160 * 1024, "encoder LDS budget");
    static_assert(!FRONT || S + RW * 33 * 16 <= FLOATS, "W + S must fit in the E0 + EB + F0 regions");
    static_assert(I % 4 == 0 && H % 4 == 0 && G % 4 == 0 && A % 4 == 0 && E % 4 == 0 && B % 4 == 0, "16B carve");
};
constexpr int ENC_LDS_FLOATS = EncLds<TC, 1, false, true>::FLOATS;
constexpr int ENC_GT_LDS_FLOATS = EncLds<TC, 1, false, false>::FLOATS;
constexpr int ENC_MS_LDS_FLOATS = EncLds<MS_ROWS, MS_STREAMS, true, true>::FLOATS;

// lens (optional, offline only): utterance b has 1 + lens[b]/256 <= T frames; T stays the row stride of every tensor.
// MS (multi-stream, single-frame streaming steps): workgroup b serves streams b*MS_STREAMS .. +3 of the NB streams,
// one new frame each; the host passes T = MS_STREAMS and the spectrogram strides sb' = MS_STREAMS * sb, st' = sb, so
// every tensor is addressed exactly as if the streams' frames were consecutive frames of "utterance" b -- only the
// history (rings, energies, frame counters) is per row.
// Q: int8-weight / fp16-activation variant (PF then holds the quantised weights); qin > 0 additionally passes the
// input spectrogram through the int8 boundary of the tflite path (x_q = round(x / qin), tflite_infer.py:79-82).
// FRONT = false (offline calls): k_front has already produced en0 and en1; this kernel reads en1 in its own slot order
// and runs only the three causal GTConv blocks.
// SPANS: the workgroups of an offline launch share the (utterance, frame) axis (see span_begin); a separate instantiation,
// so that the one-workgroup-per-utterance form (the headline shape) keeps its registers
template <int TPW, bool MS, bool Q, bool FRONT, bool SPANS = false>
__global__ __launch_bounds__(NTHR) void k_encoder(const float* __restrict__ spec, long sb, long sf, long st, int T,
                                                 const int* __restrict__ lens, int NB, float qin,
                                                 const float* __restrict__ PF, const int* __restrict__ PI,
                                                 float* __restrict__ en0, float* __restrict__ en1,
                                                 float* __restrict__ en2, float* __restrict__ en3,
                                                 float* __restrict__ en4, float* __restrict__ state,
                                                 unsigned long long* __restrict__ stamps) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    STAMP_INIT(SS)
    constexpr int RW = MS ? MS_ROWS : TC;
    constexpr int NS = MS ? MS_STREAMS : 1;
    using LD = EncLds<RW, NS, MS, FRONT>;
    constexpr int RS = LD::RS;
    static_assert(!MS || FRONT, "multi-stream steps run the whole encoder");
    float* sP = smem + LD::P;
    int* sI = reinterpret_cast<int*>(smem + LD::I);
    float* sH = smem + LD::H;
    float* sEH = smem + LD::EH;
    int* sTB = reinterpret_cast<int*>(smem + LD::TB);
    float* sG = smem + LD::G;
    float* sSpec = smem + LD::A;     // [3: mag, re, im][tl][257]
    float* sE0 = smem + LD::A;
    float* sW = smem + LD::A;
    float* sS = smem + LD::S;
    float* sEB = smem + LD::B;
    float* sF0 = sEB + 3 * RW * EB_ROW;
    const Lane L = lane_info();
    const int tid = L.tid, n = L.n, g = L.g;
    // offline calls (no stream state, no per-utterance lengths, FRONT = false): the workgroups share the (utterance,
    // frame) axis, a share is a run of segments (see span_begin / span_next); everything else: one workgroup per utterance / stream
    const int Tstride = T;
    static_assert(!SPANS || (!MS && !FRONT), "time spans: offline blocks-only form");
    SpanIter sit;
    #ifdef GT_EXP_SAMEUTT    // timing experiment only (wrong results): every workgroup works on one of eight utterances, so all
    int s_b = blockIdx.x & 7, s_fb = 0, s_wlo = 0, s_nT = T;   // hand-off traffic hits in L2: the kernels without HBM latency
#else
    int s_b = blockIdx.x, s_fb = 0, s_wlo = 0, s_nT = T;
#endif
    if constexpr (SPANS) {     // (`lens` is the PREFIX table of a variable-length batch here, see span_begin)
        if (!span_begin(sit, blockIdx.x, gridDim.x, NB, T, lens)) return;
        span_next(sit, NB, Tstride, lens, HALO_BLOCKS, s_b, s_fb, s_wlo, s_nT);
    }
    int b = s_b;

    static_assert(E_BLK % 4 == 0 && ENC_SIZE % 4 == 0 && P_ENC % 4 == 0, "16-byte parameter copies");
    copy_params(sP + (FRONT ? 0 : E_BLK), PF + P_ENC + (FRONT ? 0 : E_BLK), ENC_SIZE - (FRONT ? 0 : E_BLK), tid, NTHR);
    // the integer tables without the decoder-side ERB.bs index ranges (I_BS_LO, I_BS_N): [0, I_BS_LO) stays in place,
    // [I_ENC_BLK, P_INTS) moves down by ENC_I_SKIP
    for (int i = tid; i < P_INTS - ENC_I_SKIP; i += NTHR) sI[i] = PI[i < I_BS_LO ? i : i + ENC_I_SKIP];
    // (the pad entries of EB / F0 are zeroed at the top of every chunk; nothing else of that region is read unwritten)
    float* stb = state ? state + (long)b * NS * ST_FLOATS : nullptr;    // first stream of this workgroup
    const int nlive = MS ? min(NS, NB - b * NS) : 1;
    int tbase = 0;
    if constexpr (MS) {
        rings_load_ms<NS>(sH, sEH, stb, ST_ENC_H, ST_ENC_E, nlive, tid);
        if (tid < 8) sTB[tid] = tid < nlive ? reinterpret_cast<const int*>(stb + (long)tid * ST_FLOATS)[0] : 0;
    } else {
        tbase = stb ? reinterpret_cast<const int*>(stb)[0] : 0;
        rings_load(sH, sEH, stb ? stb + ST_ENC_H : nullptr, stb ? stb + ST_ENC_E : nullptr, tbase, tid);
    }
    const Tiles<TPW> tt = make_tiles<TPW>(L);
    wg_barrier();
    if constexpr (!FRONT) ring_to_image<RS, LD::PT>(sW, sH, tid);   // block 0's history of the first chunk (later ones: block 2)

    spec += (long)b * sb;
    // global addressing: wave-uniform base pointers (SGPR pairs) + 32-bit per-lane offsets; per segment: the segment's
    // first row of the hand-off tensors, its frame count T and the first local frame that is stored (wlo)
    using ht = typename HandOff<Q>::t;
    long ob;
    ht *en0h, *en1h, *en2h, *en3h, *en4h;
    const ht* x1h;                              // FRONT = false: k_front's en1 (decoder slot order), read here
    int wlo_v;
    auto seg_setup = [&](int sb_, int sfb, int swlo, int snT) {
        b = sb_;
        ob = (long)sb_ * Tstride + sfb;
        en0h = reinterpret_cast<ht*>(en0) + ob * (F1 * 16);
        en1h = reinterpret_cast<ht*>(en1) + ob * 528;
        en2h = reinterpret_cast<ht*>(en2) + ob * 528;
        en3h = reinterpret_cast<ht*>(en3) + ob * 528;
        en4h = reinterpret_cast<ht*>(en4) + ob * 528;
        x1h = reinterpret_cast<const ht*>(en1) + ob * 528;
        T = snT;
        wlo_v = swlo;
    };
    seg_setup(s_b, s_fb, s_wlo, s_nT);
    const bool t_fast = st < sf;  // reference layout (B,257,T,2): consecutive frames are adjacent
    if constexpr (!SPANS) {
        if (lens) T = min(T, 1 + (lens[b] >> 8));   // from here on T = this utterance's frames
    }
    if constexpr (MS) T = nlive;                // one frame per live stream = nlive rows
    STAMP(SS, 0)

    // Spectrogram items of this thread: item q is element idx = tid + q*NTHR of the chunk, idx -> (tl, f)
    // with f fastest for the frame-major layout (consecutive bins adjacent) and tl fastest for the
    // reference layout (consecutive frames adjacent).  The chunk is fetched one chunk ahead into
    // registers, so its HBM latency is hidden behind the previous chunk's compute.
    constexpr int SPEC_ITEMS = FRONT ? (RW * NBINS + NTHR - 1) / NTHR : 1;
    float2 spn[SPEC_ITEMS];
    const int sf32 = (int)sf, st32 = (int)st;     // api.cpp checks that a chunk's offsets fit in 31 bits
    auto spec_fetch = [&](int t0f) {
        const int nf = min(RW, T - t0f);
        const float* base = spec + (long)t0f * st;           // wave-uniform
        int tv0 = tid;
        asm volatile("" : "+v"(tv0));   // recomputed per chunk: keeps the item coordinates out of long-lived registers
        int tl, f;
        spec_item_first(tv0, t_fast, tl, f);
#pragma unroll
        for (int q = 0; q < SPEC_ITEMS; ++q) {
            const bool ok = tl < nf && f < NBINS;            // clamped: no select behind the load
            spn[q] = *reinterpret_cast<const float2*>(base + (ok ? f * sf32 + tl * st32 : 0));
            spec_item_next(t_fast, tl, f);
        }
    };
    if constexpr (FRONT) spec_fetch(0);
    // FRONT = false: the block input of the chunk, fetched one chunk ahead (clamped: no select behind the loads)
    f32x4 xn[TPW];
segment_top:
    if constexpr (!FRONT) {
        const int np0 = min(RW, T) * 33;
#pragma unroll
        for (int i = 0; i < TPW; ++i) xn[i] = ldx<Q>(x1h + (unsigned)((tt.pp(i) < np0 ? tt.pp(i) : 0) * 16 + 4 * g));
    }

    for (int t0 = 0; t0 < T; t0 += RW) {
        const int nfr = min(RW, T - t0);
        const int wlo = SPANS ? wlo_v : 0;      // first local frame that is stored (0 unless this is a warmed-up segment)
        f32x4 x[TPW];
        if constexpr (!FRONT) {
            // en1 exists only in the slot order of its decoder consumer (k_front is sensitive to its output stores: a second
            // copy in this stage's order cost it 11 %): back to the own order through the tile's scratch records
            // (S is dead at the top of a chunk)
            {
                const int* ix = sI + I_ENST - ENC_I_SKIP + 0 * 16 + 4 * g;
                int po[TPW];
#pragma unroll
                for (int i = 0; i < TPW; ++i) po[i] = tt.pp(i) * PERM_RS;
                unpermute_tiles_via_lds<TPW>(sS, po, ix, g, xn, x);
            }
            if (t0 + RW < T) {
                const int npn = min(RW, T - t0 - RW) * 33;
                const ht* xc = x1h + (long)(t0 + RW) * 528;
#pragma unroll
                for (int i = 0; i < TPW; ++i) xn[i] = ldx<Q>(xc + (unsigned)((tt.pp(i) < npn ? tt.pp(i) : 0) * 16 + 4 * g));
            }
        }
        if constexpr (FRONT) {
        // the cooperative loops index from an opaque copy of tid so that their per-item offsets are
        // recomputed per chunk instead of being hoisted, spilled and reloaded (scratch shares vmcnt)
        int tv = tid;
        asm volatile("" : "+v"(tv));
        // the EB/F0 region doubles as the scratch of the en1 store (phase D), so the zero pad entries
        // (EB columns 0 and 130, F0 columns 0,1 and 131..135) are re-zeroed every chunk
        if (tv < 3 * RW * 9) {
            const int row = tv / 9, e = tv - row * 9;
            float z = 0.f;
            asm volatile("" : "+v"(z));
            if (e < 2) sEB[row * EB_ROW + e * 130] = z;
            else sF0[row * F0_ROW + (e < 4 ? e - 2 : 127 + e)] = z;
        }
        // ---- A0: stage [mag, re, im] of the chunk in LDS; the magnitude (models/gtcrn_micro.py:514) is
        //      computed once per bin here.  The 65 pass-through bins of ERB.bm (:63-67) go straight to
        //      their place in EB; the 192 high bins are staged as [c][tl][257] for the band filters -------
        {
            int tl, f;
            spec_item_first(tv, t_fast, tl, f);
#pragma unroll
            for (int q = 0; q < SPEC_ITEMS; ++q) {
                if (tl < nfr && f < NBINS) {
                    float2 v = spn[q];
                    if constexpr (Q) {
                        if (qin > 0.f) {
                            v.x = fminf(fmaxf(rintf(v.x / qin), -128.f), 127.f) * qin;
                            v.y = fminf(fmaxf(rintf(v.y / qin), -128.f), 127.f) * qin;
                        }
                        v.x = rq1<Q>(v.x);
                        v.y = rq1<Q>(v.y);
                    }
                    const bool low = f < ERB_LOW;
                    float* d = low ? sEB + tl * EB_ROW + 1 + f : sSpec + tl * NBINS + f;
                    const int cs = low ? RW * EB_ROW : RW * NBINS;
                    d[0] = rq1<Q>(__builtin_amdgcn_sqrtf(v.x * v.x + v.y * v.y + 1e-12f));
                    d[cs] = v.x;
                    d[2 * cs] = v.y;
                }
                spec_item_next(t_fast, tl, f);
            }
        }
        STAMP(SS, 10)
        if (t0 + RW < T) spec_fetch(t0 + RW);
        STAMP(SS, 11)
        wg_barrier();
        STAMP(SS, 12)
        // ---- A: ERB.bm bands: EB[c][tl][66 + band]; items run over all RW rows of the chunk image
        //      (rows past a short last chunk are skipped).  NTHR is a multiple of
        //      64, so a lane keeps its band for all its items: the band's weights are read once per chunk -----
        {
            static_assert(NTHR % ERB_BANDS == 0, "lane <-> band");
            const int band = tv & (ERB_BANDS - 1);
            const int lo = sI[I_ERB_LO + band], cnt = sI[I_ERB_N + band];
            float w[ERB_MAXBW];
#pragma unroll
            for (int i = 0; i < ERB_MAXBW; i += 4) {
                const f32x4 t = ld4(sP + E_ERB_W + band * ERB_MAXBW + i);
                // taps beyond the band's width may read stale LDS past the row, which need not be finite:
                // they are selected away below rather than multiplied by their zero weight
                w[i] = t[0]; w[i + 1] = t[1]; w[i + 2] = t[2]; w[i + 3] = t[3];
            }
            for (int ct = tv >> 6; ct < 3 * RW; ct += NW) {
                if ((ct % RW) >= nfr) continue;
                const float* sp = sSpec + ct * NBINS + ERB_LOW + lo;
                float a0 = 0.f, a1 = 0.f;
#pragma unroll
                for (int i = 0; i < ERB_MAXBW; i += 2) {    // fixed trip count: all 12 LDS reads issue at once
                    a0 += w[i] * (i < cnt ? sp[i] : 0.f);
                    a1 += w[i + 1] * (i + 1 < cnt ? sp[i + 1] : 0.f);
                }
                sEB[ct * EB_ROW + 1 + ERB_LOW + band] = rq1<Q>(a0 + a1);
            }
        }
        STAMP(SS, 13)
        wg_barrier();
        STAMP(SS, 1)
        // ---- B: SFE_Lite depthwise (1,3): F0[c][tl][2 + f]; one (channel, frame) row per wave pass -------
        for (int row = L.wave; row < 3 * RW; row += NW) {
            const int tl = row % RW, c = row / RW;
            if (tl >= nfr) continue;
            const float w0 = sP[E_SFE_W + c * 3], w1 = sP[E_SFE_W + c * 3 + 1], w2 = sP[E_SFE_W + c * 3 + 2];
            const float* e = sEB + row * EB_ROW;
            float* d = sF0 + row * F0_ROW + 2;
            // 129 bins = 2 x 64 lanes + 1: the last bin rides on lane 0 instead of a third, nearly empty pass
            static_assert(F0 == 129, "SFE lane mapping");
            const int f = tv & 63;
            d[f] = rq1<Q>(w0 * e[f] + w1 * e[f + 1] + w2 * e[f + 2]);
            d[f + 64] = rq1<Q>(w0 * e[f + 64] + w1 * e[f + 65] + w2 * e[f + 66]);
            if (f == 0) d[128] = rq1<Q>(w0 * e[128] + w1 * e[129] + w2 * e[130]);
        }
        // zero the pad positions of E0 (columns 0,1,67,68 of each row): region A held the spectrogram
        if (tv < RW * 4 * 4) {
            const int r = tv >> 4, cc = (tv >> 2) & 3, gg = tv & 3;
            float z = 0.f;
            asm volatile("" : "+v"(z));
            st4(sE0 + pl(r * ENC_E0_ROW + (cc < 2 ? cc : 65 + cc), gg), splat(z));
        }
        wg_barrier();
        STAMP(SS, 2)
        // ---- C: en_convs.0 = Conv2d(3,16,(1,5),stride (1,2),pad (0,2)) + BN + PReLU --------------
        {
            const f32x4 A = ld4(sP + E_EN0_A + arow(n, g)), Bv = ld4(sP + E_EN0_B + 4 * g);
            const float a = slope_arg<Q>(sP[E_EN0_S]);
            int off[4];
            int go = g;
            asm volatile("" : "+v"(go));   // recompute the im2col offsets per chunk instead of spilling them
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int e = 4 * go + s, c = e < 15 ? e / 5 : 0, k = e < 15 ? e % 5 : 0;
                off[s] = c * RW * F0_ROW + k;
            }
            static_assert(TC * F1 % 16 == 0, "en0 tiling");
            const int nt0 = (nfr * F1 + 15) >> 4;              // tiles that hold a valid frame
            for (int tile = L.wave; tile < nt0; tile += NW) {
                const int q = tile * 16 + n;
                int tl = q / F1;
                const int fo = q - tl * F1;
                if (MS && tl >= RW) tl = RW - 1;               // tail lanes of the last tile: stay inside the images
                f32x4 bv;
#pragma unroll
                for (int s = 0; s < 4; ++s) bv[s] = sF0[off[s] + tl * F0_ROW + 2 * fo];
                f32x4 acc = mm1<Q>(A, bv, Bv);
                acc = rq<Q>(prelu4q<Q>(acc, a));
                st4(sE0 + pl(tl * ENC_E0_ROW + 2 + fo, g), acc);
                if (q < nfr * F1) stx<Q>(en0h + (long)t0 * (F1 * 16) + (unsigned)(q * 16 + 4 * g), acc);
            }
        }
        wg_barrier();
        STAMP(SS, 3)
        // ---- D: en_convs.1 = Conv2d(16,16,(1,5),stride (1,2),pad (0,2)) + BN + PReLU -------------
        {
            const f32x4 Bv = ld4(sP + E_EN1_B + 4 * g);
            const float a = slope_arg<Q>(sP[E_EN1_S]);
            const int* ix = sI + I_ENST - ENC_I_SKIP + 0 * 16 + 4 * g;
            // tap major: each of the five 16x16 slot matrices is read from LDS once per wave, one MFMA chain per tile
#pragma unroll
            for (int i = 0; i < TPW; ++i) x[i] = Bv;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const f32x4 A = ld4(sP + E_EN1_A + k * 256 + arow(n, g));
#pragma unroll
                for (int i = 0; i < TPW; ++i) {
                    const f32x4 tap = ld4(sE0 + pl(tt.tl[i] * ENC_E0_ROW + 2 * tt.ff[i], g) + k * 16);
                    x[i] = mm1<Q>(A, tap, x[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                x[i] = rq<Q>(prelu4q<Q>(x[i], a));
                {   // en1 in the slot order of its decoder consumer; scratch: this tile's records of F0/EB (dead)
                    const f32x4 y = permute_via_lds(sEB + tt.pp(i) * 16, ix, g, x[i]);
                    if (tt.pp(i) < nfr * 33 && t0 + tt.tl[i] >= wlo) stx<Q>(en1h + (long)t0 * 528 + (unsigned)(tt.pp(i) * 16 + 4 * g), y);
                }
            }
        }
        wg_barrier();  // E0 is dead: its region becomes W
        STAMP(SS, 4)
        }   // FRONT
        zero_row_pads<LD::RWI, RS, LD::PT>(sW, tid);
        // ---- E: 3 x GTConvBlock (depthwise) --------------------------------------------------------
#pragma unroll 1
        for (int k = 0; k < 3; ++k) {
            BlockCtx c;
            c.pb = sP + E_BLK + k * GB_SIZE;
            c.gA = nullptr;
            c.ib = sI + I_ENC_BLK - ENC_I_SKIP + k * 16;
            c.sW = sW; c.sHk = sH + k * RING_DENSE; c.sS = sS; c.sG = sG; c.sEHk = sEH + k * 16;
            // FRONT: region A held the staged spectrogram / E0 until this chunk's phase D, so block 0 fetches its
            // history itself; otherwise the image is only ever W and block 2 prepares the next chunk's block 0
            c.sHtop = FRONT && k == 0 ? sH : nullptr;
            c.sHnext = k < 2 ? sH + (k + 1) * RING_DENSE : (FRONT ? nullptr : sH);
            c.sE = smem + LD::E;
            c.sY = sG + RW * 16;
            c.nfr = nfr; c.tabs = tbase + t0;
            c.sTB = sTB;
            if constexpr (MS) {
                const int sidx = min(tt.tl[0], NS - 1);
                c.ms_roff[0] = (int)(sH - sW) + sidx * RING_SET + k * (2 * 35 * 16);
                c.ms_tb[0] = sTB[sidx];
            } else {
                c.ms_roff[0] = 0; c.ms_tb[0] = 0;
            }
            c.g_hist[0] = nullptr;
            gtconv_block<false, TPW, MS, Q, RS, RS, !(FRONT && TPW == 3), LD::PT>(x, tt, c, L, [] {}, [] {} STAMP_ARG);
            if (k < 2) {
                ht* dst = k == 0 ? en2h : en3h;
                const int* ix = sI + I_ENST - ENC_I_SKIP + (k + 1) * 16 + 4 * g;
                // scratch: the tiles' own v^2 records (dead after the gate barrier)
                if constexpr (!FRONT) {
                    int po[TPW];
                    f32x4 y[TPW];
#pragma unroll
                    for (int i = 0; i < TPW; ++i) po[i] = tt.pp(i) * PERM_RS;
                    permute_tiles_via_lds<TPW>(sS, po, ix, g, x, y);
#pragma unroll
                    for (int i = 0; i < TPW; ++i)
                        if (tt.pp(i) < nfr * 33 && t0 + tt.tl[i] >= wlo) stx<Q>(dst + (long)t0 * 528 + (unsigned)(tt.pp(i) * 16 + 4 * g), y[i]);
                } else {   // (the streaming forms carry the front end's registers: one tile at a time)
#pragma unroll
                    for (int i = 0; i < TPW; ++i) {
                        const f32x4 y = permute_via_lds(sS + tt.pp(i) * PERM_RS, ix, g, x[i]);
                        if (tt.pp(i) < nfr * 33 && t0 + tt.tl[i] >= wlo) stx<Q>(dst + (long)t0 * 528 + (unsigned)(tt.pp(i) * 16 + 4 * g), y);
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < TPW; ++i)
                    if (tt.pp(i) < nfr * 33 && t0 + tt.tl[i] >= wlo) stx<Q>(en4h + (long)t0 * 528 + (unsigned)(tt.pp(i) * 16 + 4 * g), x[i]);
            }
            STAMP(SS, 8)
        }
        wg_barrier();  // region A is rewritten (staged spectrogram) by the next chunk
        STAMP(SS, 9)
    }
    if constexpr (SPANS) {
        if (span_next(sit, NB, Tstride, lens, HALO_BLOCKS, s_b, s_fb, s_wlo, s_nT)) {
            // the share runs on into the next utterance: zero history again (every wave is behind the barrier that closed
            // the last chunk, i.e. behind all reads of the rings and images), then the same chunk loop
            rings_load(sH, sEH, nullptr, nullptr, 0, tid);
            wg_barrier();
            ring_to_image<RS, LD::PT>(sW, sH, tid);
            seg_setup(s_b, s_fb, s_wlo, s_nT);
            goto segment_top;
        }
    }
    if (stb) {
        wg_barrier();
        if constexpr (MS) {
            rings_store_ms<NS>(sH, sEH, stb, ST_ENC_H, ST_ENC_E, nlive, tid);
        } else {
            rings_store(sH, sEH, stb + ST_ENC_H, stb + ST_ENC_E, tbase + T, tid);
        }
    }
    STAMP_OUT(SS, stamps)
}

// (Two other workgroup shapes of these three blocks were built on the same gtconv_block in round 5 -- two six-wave
// workgroups per CU over 512 shares, and sixteen waves with two tiles each -- measured same-box, bit-identical, not faster
// (0.268 / 0.2068 ms against 0.214 / 0.2063 ms), and removed from the source in round 6: profiles/r05_ab_encoder_forms.txt.
// gtconv_block keeps the NWV / PMAX template arguments they introduced: the wide streaming step uses them.)

// =============================================================================== front end (offline form)
// Everything in front of the first GTConv block has NO dependence across frames: reflect-pad framing, window, FFT
// (infer.py:60-67), [mag,re,im] (models/gtcrn_micro.py:510-515), ERB.bm (:63-67), SFE_Lite (:77-90) and the two
// strided (1,5) ConvBlocks (:344-364).  Offline calls therefore run it as a THROUGHPUT kernel instead of inside the
// lock-stepped per-utterance encoder: ONE FRAME PER WAVE from the waveform samples to en1, in 7.6 KB of wave-private
// LDS, so the waves never meet at a barrier (persistent workgroups of eight waves, two per CU = 4 waves per SIMD: three per SIMD measured 40 % slower,
// parameters copied to LDS once).  The frame never leaves LDS between the FFT and the convs; the spectrogram is
// also written out once (the decoder's mask multiplies it).  Price: a frame's 65 / 33 positions fill 5 / 3 MFMA
// tiles (80 MFMAs per frame instead of 59 for tiles cut across frames).  Same source expressions as k_encoder's
// in-kernel front end (which the streaming forms keep), so every value is bit-identical.
// WAVE_IN = false: the frames come from a caller spectrogram (gtcrn_forward_spec) instead of the FFT.
// Outputs: the spectrogram, en0 (B,T,65,16) and en1 (B,T,33,16) in the slot order of its decoder consumer (en1p);
// the first GTConv block un-permutes it on load.  The kernel is sensitive to these stores (0.53 GB per launch at
// B = 256 x 4 s: a second copy of en1 in its own slot order made it 11 % slower).
constexpr int FR_WAVES = 8;
constexpr int FR_NT = FR_WAVES * 64;
constexpr int FR_P = 0;                                        // E_ERB_W .. E_BLK of the encoder segment
constexpr int FR_I = FR_P + ((E_BLK + 3) & ~3);                // I_ERB_LO[64], I_ERB_N[64], I_ENST[0][16] (+pad)
constexpr int FR_TW = FR_I + 160;                              // twiddles 256 + 256 complex, window 512
constexpr int FR_W0 = FR_TW + 1536;                            // wave-private regions start here
constexpr int FR_WX = 0;                                       // FFT ping (512) + pong (512, later the staged high bins), later E0 [69][16]
constexpr int FR_WEB = FR_WX + ENC_E0_ROW * 16;                // EB [3][131] (+3 pad)
constexpr int FR_WF0 = FR_WEB + 396;                           // F0 [3][136]; EB..F0 later the en1 permute scratch
constexpr int FR_WSZ = FR_WF0 + 3 * F0_ROW;
constexpr int FR_LDS_FLOATS = FR_W0 + FR_WAVES * FR_WSZ;
static_assert(1024 <= ENC_E0_ROW * 16 && 2 * 192 <= 512, "FFT buffers / staged high bins must fit in the E0 region");
static_assert(3 * 16 * 16 <= 396 + 3 * F0_ROW, "en1 permute scratch (3 tiles) must fit in EB + F0");
static_assert(3 * 16 * PERM_RS <= ENC_E0_ROW * 16, "en1 permute scratch (3 tiles) must fit in the E0 region");
static_assert(FR_W0 % 4 == 0 && FR_WSZ % 4 == 0 && FR_WEB % 4 == 0 && FR_WF0 % 4 == 0, "16B carve");
static_assert(FR_LDS_FLOATS * 4 * 2 <= 160 * 1024, "two front-end workgroups per CU");

template <bool WAVE_IN, bool Q>
__global__ __launch_bounds__(FR_NT, 4) void k_front(const float* __restrict__ in, long L, long isb, long isf, long ist,
                                                int B, int T, const int* __restrict__ lens,
                                                const float* __restrict__ win, const float2* __restrict__ twid,
                                                const float* __restrict__ PF, const int* __restrict__ PI,
                                                float* __restrict__ spec, float* __restrict__ en0,
                                                float* __restrict__ en1p, float qin) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sP = smem + FR_P;                   // indexed with the E_* offsets of the encoder segment
    int* sI = reinterpret_cast<int*>(smem + FR_I);
    float2* s_tw = reinterpret_cast<float2*>(smem + FR_TW);
    float2* s_tw512 = s_tw + 256;
    float* s_win = smem + FR_TW + 1024;
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* mine = smem + FR_W0 + wv * FR_WSZ;
    float2* A = reinterpret_cast<float2*>(mine + FR_WX);
    float2* Bf = A + 256;                      // FFT pong buffer, then the staged (re, im) of the 192 high bins
    float* sE0 = mine + FR_WX;
    float* sEB = mine + FR_WEB;
    float* sF0 = mine + FR_WF0;
    copy_params(sP, PF + P_ENC, E_BLK, tid, FR_NT);
    for (int i = tid; i < 128; i += FR_NT) sI[i] = PI[I_ERB_LO + i];
    if (tid < 16) sI[128 + tid] = PI[I_ENST + tid];
    if (WAVE_IN) fft_tables_load(s_tw, s_tw512, s_win, twid, win, tid, FR_NT);
    __syncthreads();          // the only workgroup barrier: from here on every wave works on its own frames
    const long nframes = (long)B * T, stride = (long)gridDim.x * FR_WAVES;
    long fr = (long)blockIdx.x * FR_WAVES + wv;
    // frame `fr` of the flattened (utterance, frame) axis is frame t of utterance b.  fr advances by the constant
    // `stride`, so (b, t) are divided out ONCE and then stepped by (stride / T, stride % T) with one carry; with
    // per-utterance lengths the frames past an utterance's end do not exist (skipped), and an utterance's length is
    // read when b changes, not per frame.
    int b = (int)(fr / T), t = (int)(fr - (long)b * T);
    const int step_b = (int)(stride / T), step_t = (int)(stride - (long)step_b * T);
    int b_len = -1;                            // the utterance Lb belongs to
    long Lb = L;
    // (a lambda, as the fetch always was: it is inlined after the frame loop is simplified, not ahead of it as a forced
    // inline in the loop would be, and the kernel's instructions stay what they were)
    auto fetch = [&](int b, int t, long Lb, float2 (&v)[4]) { frame_fetch(in + (long)b * L, t, Lb, lane, v); };
    // bin k of the frame -> the LDS images: low bins straight to their place in EB (ERB.bm passes them through),
    // high bins as (re, im) pairs for the band filters; the magnitude of a high bin is formed where it is used
    auto quant_in = [&](float2 v) -> float2 {
        if constexpr (Q) {
            if (qin > 0.f) {
                v.x = fminf(fmaxf(rintf(v.x / qin), -128.f), 127.f) * qin;
                v.y = fminf(fmaxf(rintf(v.y / qin), -128.f), 127.f) * qin;
            }
            v.x = rq1<Q>(v.x);
            v.y = rq1<Q>(v.y);
        }
        return v;
    };
    auto stage = [&](int k, float2 v) {
        v = quant_in(v);
        if (k < ERB_LOW) {
            float* d = sEB + 1 + k;
            d[0] = rq1<Q>(__builtin_amdgcn_sqrtf(v.x * v.x + v.y * v.y + 1e-12f));
            d[EB_ROW] = v.x;
            d[2 * EB_ROW] = v.y;
        } else {
            Bf[k - ERB_LOW] = v;
        }
    };
    float2 cur[4];
    // the frame's records in the three outputs, as byte offsets from the frame's first byte: the frame bases are wave
    // uniform (scalar registers, stepped by the loop), so a store is base + 32-bit lane offset with no 64-bit vector
    // pointer formed per store
    using ht = typename HandOff<Q>::t;
    constexpr unsigned EB = (unsigned)sizeof(ht);
    const unsigned rec_off = (unsigned)(n * 16 + 4 * g) * EB;      // record n, slot group g, of a tile's first record
    // ERB.bm: the band's first bin and width (lane = band) do not change from frame to frame
    const int erb_lo = sI[lane], erb_cnt = sI[64 + lane];
    for (; fr < nframes; fr += stride, b += step_b, t += step_t) {
        if (t >= T) { t -= T; ++b; }
        if (lens && b != b_len) { Lb = (long)lens[b]; b_len = b; }
        const bool live = !lens || t <= (int)(Lb >> 8);
        // (no prefetch of the next frame: four waves per SIMD hide the load, and its eight registers would spill)
        if (WAVE_IN && live) fetch(b, t, Lb, cur);
        if (live) {
            // ---- the frame -> [mag, re, im] in LDS (+ the spectrogram written out) --------------------------------
            if constexpr (WAVE_IN) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int m = lane + 64 * q;
                    A[m] = frame_window(cur[q], s_win, m);
                }
                wave_lds_sync();
                fft256<-1>(A, Bf, s_tw, lane);
                float* o = spec + fr * (2 * NBINS);               // frame-major (B,T,257,2)
                float2 X[4], XN = make_float2(0.f, 0.f);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int k = lane + 64 * q;
                    const float2 zk = A[k];
                    X[q] = rfft_bin(A, s_tw512, k, zk);
                    if (k == 0) XN = rfft_nyquist(zk);
                }
                wave_lds_sync();                                  // every lane has read A and Bf is free: stage
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int k = lane + 64 * q;
                    { const f32x2 xv = {X[q].x, X[q].y}; __builtin_nontemporal_store(xv, reinterpret_cast<f32x2*>(o + 2 * k)); }
                    stage(k, X[q]);
                }
                if (lane == 0) {
                    *reinterpret_cast<float2*>(o + 2 * 256) = XN;
                    stage(256, XN);
                }
            } else {
                const float* base = in + (long)b * isb + (long)t * ist;
                for (int k = lane; k < NBINS; k += 64) stage(k, *reinterpret_cast<const float2*>(base + (long)k * isf));
            }
            if (lane < 6) sEB[(lane >> 1) * EB_ROW + (lane & 1) * 130] = 0.f;     // EB pad columns 0 and 130
            wave_lds_sync();
            // ---- A: ERB.bm: lane = band; the three channels share the band's (re, im) reads ----------------------
            {
                const int band = lane;
                const int lo = erb_lo, cnt = erb_cnt;
                float w[ERB_MAXBW];
#pragma unroll
                for (int i = 0; i < ERB_MAXBW; i += 4) {
                    const f32x4 tq = ld4(sP + E_ERB_W + band * ERB_MAXBW + i);
                    w[i] = tq[0]; w[i + 1] = tq[1]; w[i + 2] = tq[2]; w[i + 3] = tq[3];
                }
                float m0 = 0.f, m1 = 0.f, r0 = 0.f, r1 = 0.f, i0 = 0.f, i1 = 0.f;
#pragma unroll
                for (int i = 0; i < ERB_MAXBW; i += 2) {        // taps beyond the band's width are selected away
                    const float2 va = Bf[(lo + i) & 255], vb = Bf[(lo + i + 1) & 255];
                    const float ma = rq1<Q>(__builtin_amdgcn_sqrtf(va.x * va.x + va.y * va.y + 1e-12f));
                    const float mb = rq1<Q>(__builtin_amdgcn_sqrtf(vb.x * vb.x + vb.y * vb.y + 1e-12f));
                    m0 += w[i] * (i < cnt ? ma : 0.f);
                    m1 += w[i + 1] * (i + 1 < cnt ? mb : 0.f);
                    r0 += w[i] * (i < cnt ? va.x : 0.f);
                    r1 += w[i + 1] * (i + 1 < cnt ? vb.x : 0.f);
                    i0 += w[i] * (i < cnt ? va.y : 0.f);
                    i1 += w[i + 1] * (i + 1 < cnt ? vb.y : 0.f);
                }
                float* d = sEB + 1 + ERB_LOW + band;
                d[0] = rq1<Q>(m0 + m1);
                d[EB_ROW] = rq1<Q>(r0 + r1);
                d[2 * EB_ROW] = rq1<Q>(i0 + i1);
            }
            wave_lds_sync();
            // ---- B: SFE_Lite (same row code as k_encoder) ---------------------------------------------------------
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float w0 = sP[E_SFE_W + c * 3], w1 = sP[E_SFE_W + c * 3 + 1], w2 = sP[E_SFE_W + c * 3 + 2];
                const float* e = sEB + c * EB_ROW;
                float* d = sF0 + c * F0_ROW + 2;
                const int f = lane;
                d[f] = rq1<Q>(w0 * e[f] + w1 * e[f + 1] + w2 * e[f + 2]);
                d[f + 64] = rq1<Q>(w0 * e[f + 64] + w1 * e[f + 65] + w2 * e[f + 66]);
                if (f == 0) d[128] = rq1<Q>(w0 * e[128] + w1 * e[129] + w2 * e[130]);
                if (f < 7) d[(f < 2 ? f - 2 : 127 + f)] = 0.f;   // columns 0,1 and 131..135 of the row
            }
            // zero the pad positions of E0 (columns 0,1,67,68): the region held the FFT buffers / staged bins
            if (lane < 16) st4(sE0 + pl(((lane >> 2) < 2 ? (lane >> 2) : 65 + (lane >> 2)), lane & 3), splat(0.f));
            wave_lds_sync();
            // ---- C: en_convs.0: 65 positions = 5 tiles (the last one holds a single valid position) ---------------
            {
                const f32x4 Am = ld4(sP + E_EN0_A + arow(n, g)), Bv = ld4(sP + E_EN0_B + 4 * g);
                const float a = slope_arg<Q>(sP[E_EN0_S]);
                int off[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int e = 4 * g + s, c = e < 15 ? e / 5 : 0, k = e < 15 ? e % 5 : 0;
                    off[s] = c * F0_ROW + k;
                }
                char* en0c = reinterpret_cast<char*>(reinterpret_cast<ht*>(en0) + fr * (F1 * 16));
#pragma unroll
                for (int tile = 0; tile < 5; ++tile) {
                    const int q = tile * 16 + n;
                    const int fo = q < F1 ? q : F1 - 1;          // tail lanes of the last tile recompute bin 64 (not stored)
                    f32x4 bv;
#pragma unroll
                    for (int s = 0; s < 4; ++s) bv[s] = sF0[off[s] + 2 * fo];
                    f32x4 acc = mm1<Q>(Am, bv, Bv);
                    acc = rq<Q>(prelu4q<Q>(acc, a));
                    if (q < F1) {
                        st4(sE0 + pl(2 + fo, g), acc);
                        stx<Q>(reinterpret_cast<ht*>(en0c + (rec_off + (unsigned)(tile * 256) * EB)), acc);
                    }
                }
            }
            wave_lds_sync();
            // ---- D: en_convs.1: 33 positions = 3 tiles; stored in both slot orders ---------------------------------
            {
                const f32x4 Bv = ld4(sP + E_EN1_B + 4 * g);
                const float a = slope_arg<Q>(sP[E_EN1_S]);
                const int* ix = sI + 128 + 4 * g;
                char* en1pc = reinterpret_cast<char*>(reinterpret_cast<ht*>(en1p) + fr * 528);
                f32x4 x[3];
                int ffv[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const int p = i * 16 + n;
                    ffv[i] = p < 33 ? p : 32;
                    x[i] = Bv;
                }
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    const f32x4 Am = ld4(sP + E_EN1_A + k * 256 + arow(n, g));
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const f32x4 tap = ld4(sE0 + pl(2 * ffv[i], g) + k * 16);
                        x[i] = mm1<Q>(Am, tap, x[i]);
                    }
                }
                wave_lds_sync();                                  // EB / F0 are dead: they become the permute scratch
                {
                    int po[3];
                    f32x4 y[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        po[i] = (i * 16 + n) * PERM_RS;
                        x[i] = rq<Q>(prelu4q<Q>(x[i], a));
                    }
                    permute_tiles_via_lds<3>(sE0, po, ix, g, x, y);     // E0's taps are consumed: X region
#pragma unroll
                    for (int i = 0; i < 3; ++i)
                        if (i * 16 + n < 33) stx<Q>(reinterpret_cast<ht*>(en1pc + (rec_off + (unsigned)(i * 256) * EB)), y[i]);
                }
            }
            wave_lds_sync();     // every region is rewritten by the next frame
        }
    }
}

// ================================================================================== GTCN
// GTCN.forward = 4 x TCN (models/gtcrn_micro.py:290-336): y1 = PReLU(BN(conv1 x)); y2 =
// PReLU(BN(depthwise (3,1) dilated d over [hist(2d) | y1])); out = PReLU(BN(conv3 y2) + x).
// x stays in registers across the four blocks; only y1 goes through LDS (chunk image sW plus a
// 2d-row ring per block, row = frame mod 2d).
constexpr int GT_LDS_P = 0;
constexpr int GT_LDS_W = GT_LDS_P + GTCN_SIZE;             // two chunk images, used alternately by the blocks
constexpr int GT_LDS_H = GT_LDS_W + 2 * TC * 33 * 16;
constexpr int GT_LDS_FLOATS = GT_LDS_H + 30 * 33 * 16;
static_assert(GT_LDS_W % 4 == 0, "16B carve");
static_assert(GT_LDS_FLOATS * 4 <= 160 * 1024, "GTCN LDS budget");

// one TCN block, dilation D (compile time); own = float offset of the lane's record in a chunk image.
// ONE barrier per block: taps older than the chunk come from the block's ring and are read BEFORE the
// barrier (they do not depend on this block's y1, and their latency hides behind conv1); the ring is
// rewritten after the barrier, when every wave is past its ring reads; the chunk image alternates
// between two buffers so that the next block's y1 never overwrites taps a slower wave still reads.
// GRING: sHk points at the stream's ring in GLOBAL memory (short streaming calls: no LDS copy of the 63 KB of
// rings).  The ring rows written after the barrier were read by other waves before it, so those loads must have
// returned (vmcnt) before any wave passes the barrier.
template <int D, bool GRING, int TPW>
__device__ __forceinline__ void tcn_block(f32x4 (&x)[TPW], const float* pk, float* sWb, float* sHk,
                                          const int (&own)[TPW], const int (&tl)[TPW], const int (&ff)[TPW],
                                          int tb16, int nfr, int npos, const int (&pp)[TPW], const Lane& L STAMP_PARAM) {
    const int n = L.n, g = L.g;
    constexpr int M2D = 2 * D - 1;
    const float a1 = pk[TCN_SLOPE] - 1.0f, a2 = pk[TCN_SLOPE + 1] - 1.0f, a3 = pk[TCN_SLOPE + 2] - 1.0f;
    f32x4 y1[TPW], acc[TPW], tp1[TPW], tp2[TPW];
    int r2[TPW];
    // ring row of frame t is t mod 2d; chunk starts are multiples of 16 >= 2d
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int r1 = (((tb16 + tl[i] + D) & M2D) * 33 + ff[i]) * 16 + 4 * g;
        r2[i] = (((tb16 + tl[i]) & M2D) * 33 + ff[i]) * 16 + 4 * g;
        tp1[i] = ld4(sHk + r1);     // frame t-d  (used when t-d  lies before the chunk)
        tp2[i] = ld4(sHk + r2[i]);  // frame t-2d (used when t-2d lies before the chunk)
    }
    {
        const f32x4 A = ld4(pk + TCN_A1 + arow(n, g)), Bv = ld4(pk + TCN_B1 + 4 * g);
#pragma unroll
        for (int i = 0; i < TPW; ++i) acc[i] = Bv;
        mm16<TPW>(A, x, acc);
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            y1[i] = prelu4(acc[i], a1);
            st4(sWb + own[i], y1[i]);
        }
    }
    if (GRING) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else wg_barrier();
    STAMP(SS, 2)
    {
        const f32x4 w0 = ld4(pk + TCN_DW + 4 * g), w1 = ld4(pk + TCN_DW + 16 + 4 * g),
                    w2 = ld4(pk + TCN_DW + 32 + 4 * g), B2 = ld4(pk + TCN_B2 + 4 * g);
        const f32x4 A = ld4(pk + TCN_A3 + arow(n, g)), B3 = ld4(pk + TCN_B3 + 4 * g);
        f32x4 y2[TPW];
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            // in-chunk taps: lanes whose tap lies before the chunk read their own record (discarded)
            const f32x4 c1 = ld4(sWb + (tl[i] >= D ? own[i] - 33 * D * 16 : own[i]));
            const f32x4 c2 = ld4(sWb + (tl[i] >= 2 * D ? own[i] - 66 * D * 16 : own[i]));
            const f32x4 t1 = tl[i] >= D ? c1 : tp1[i];
            const f32x4 t2 = tl[i] >= 2 * D ? c2 : tp2[i];
            y2[i] = prelu4(B2 + w0 * t2 + w1 * t1 + w2 * y1[i], a2);
            acc[i] = B3 + x[i];
        }
        mm16<TPW>(A, y2, acc);
#pragma unroll
        for (int i = 0; i < TPW; ++i) x[i] = prelu4(acc[i], a3);
    }
    STAMP(SS, 3)
#pragma unroll
    for (int i = 0; i < TPW; ++i)
        if (pp[i] < npos && tl[i] >= nfr - 2 * D) st4(sHk + r2[i], y1[i]);
    STAMP(SS, 4)
}

template <int TPW, bool GRING>
__global__ __launch_bounds__(NTHR) void k_gtcn(const float* __restrict__ xin, float* __restrict__ xout,
                                              const float* __restrict__ P, int T, float* __restrict__ state,
                                              int st_off, const float* __restrict__ addend,
                                              unsigned long long* __restrict__ stamps) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    STAMP_INIT(SS)
    float* sP = smem + GT_LDS_P;
    float* sW = smem + GT_LDS_W;
    const Lane L = lane_info();
    const int tid = L.tid, n = L.n, g = L.g;
#ifdef GT_EXP_SAMEUTT
    const int b = blockIdx.x & 7;
#else
    const int b = blockIdx.x;
#endif
    copy_params(sP, P, GTCN_SIZE, tid, NTHR);
    float* stb = state ? state + (long)b * ST_FLOATS : nullptr;
    const int tbase = stb ? reinterpret_cast<const int*>(stb)[0] : 0;
    // the rings [30 rows][33][16]: an LDS copy of the stream state, or (GRING) the state itself -- same layout
    float* sH = GRING ? stb + st_off : smem + GT_LDS_H;
    if (!GRING)
        for (int i = tid; i < 30 * 33 * 4; i += NTHR) {
            const int gg = i & 3, pos = i >> 2;
            st4(sH + pl(pos, gg), stb ? ld4(stb + st_off + pos * 16 + gg * 4) : splat(0.f));
        }
    wg_barrier();
    xin += (long)b * T * 528;
    xout += (long)b * T * 528;
    if (addend) addend += (long)b * T * 528;
    int pp[TPW], tl[TPW], ff[TPW], own[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        pp[i] = (L.wave + i * NW) * 16 + n;
        tl[i] = pp[i] / 33;
        ff[i] = pp[i] - tl[i] * 33;
        own[i] = pp[i] * 16 + 4 * g;
    }
    const int tb16 = tbase & 15;
    STAMP(SS, 0)

    for (int t0 = 0; t0 < T; t0 += TC) {
        const int nfr = min(TC, T - t0), npos = nfr * 33;
        // positions past the end of the utterance load a clamped (valid) record: no select, so the
        // loads are not waited for until their first use; such lanes are never stored
        f32x4 x[TPW], ad[TPW];
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const long o = (long)t0 * 528 + (pp[i] < npos ? own[i] : 4 * g);
            x[i] = ld4(xin + o);
            if (addend) ad[i] = ld4(addend + o);
        }
        STAMP(SS, 1)
        float* sW1 = sW + TC * 33 * 16;
        tcn_block<1, GRING>(x, sP + 0 * TCN_SIZE, sW, sH + 0 * 528, own, tl, ff, tb16, nfr, npos, pp, L STAMP_ARG);
        tcn_block<2, GRING>(x, sP + 1 * TCN_SIZE, sW1, sH + 2 * 528, own, tl, ff, tb16, nfr, npos, pp, L STAMP_ARG);
        tcn_block<4, GRING>(x, sP + 2 * TCN_SIZE, sW, sH + 6 * 528, own, tl, ff, tb16, nfr, npos, pp, L STAMP_ARG);
        tcn_block<8, GRING>(x, sP + 3 * TCN_SIZE, sW1, sH + 14 * 528, own, tl, ff, tb16, nfr, npos, pp, L STAMP_ARG);
#pragma unroll
        for (int i = 0; i < TPW; ++i)
            if (pp[i] < npos) st4(xout + (long)t0 * 528 + own[i], addend ? x[i] + ad[i] : x[i]);
        STAMP(SS, 5)
    }
    STAMP_OUT(SS, stamps)
    if (stb && !GRING) {
        wg_barrier();
        for (int i = tid; i < 30 * 33 * 4; i += NTHR) {
            const int gg = i & 3, pos = i >> 2;
            st4(stb + st_off + pos * 16 + gg * 4, ld4(sH + pl(pos, gg)));
        }
    }
}

// ---------------------------------------------------------------------------- GTCN, multi-stream single-frame form
// One new frame per stream (the streaming step of gtcrn_micro_stream.py:265-350 for N streams): the TCN couples a
// position (stream, bin) only with ITS OWN history, which lives in the stream's ring in global memory -- a lane reads
// the rows of frames t-d and t-2d of its position and overwrites the row of t-2d with y1(t) (row = frame mod 2d).
// Nothing is shared between lanes: no LDS image, no barrier; a tile is 16 consecutive positions of the flattened
// (stream, bin) axis, one tile per wave, four waves per workgroup.  Same arithmetic, in the same order, as tcn_block.
constexpr int GTMS_WAVES = 4;
template <int D>
__device__ __forceinline__ void tcn_block_ms(f32x4& x, const float* pk, const f32x4 t1, const f32x4 t2, float* ring_r2,
                                             bool live, int n, int g) {
    const float a1 = pk[TCN_SLOPE] - 1.0f, a2 = pk[TCN_SLOPE + 1] - 1.0f, a3 = pk[TCN_SLOPE + 2] - 1.0f;
    f32x4 y1[1], acc[1], xx[1] = {x};
    {
        const f32x4 A = ld4(pk + TCN_A1 + arow(n, g)), Bv = ld4(pk + TCN_B1 + 4 * g);
        acc[0] = Bv;
        mm16<1>(A, xx, acc);
        y1[0] = prelu4(acc[0], a1);
    }
    {
        const f32x4 w0 = ld4(pk + TCN_DW + 4 * g), w1 = ld4(pk + TCN_DW + 16 + 4 * g),
                    w2 = ld4(pk + TCN_DW + 32 + 4 * g), B2 = ld4(pk + TCN_B2 + 4 * g);
        const f32x4 A = ld4(pk + TCN_A3 + arow(n, g)), B3 = ld4(pk + TCN_B3 + 4 * g);
        f32x4 y2[1];
        y2[0] = prelu4(B2 + w0 * t2 + w1 * t1 + w2 * y1[0], a2);
        acc[0] = B3 + x;
        mm16<1>(A, y2, acc);
        x = prelu4(acc[0], a3);
    }
    if (live) st4(ring_r2, y1[0]);
}

// BOTH stacks in one launch (x stays in registers across the eight blocks): xout1 = gtcn1(xin) (kept for the stage
// taps), xout2 = gtcn2(gtcn1(xin)) + xin, exactly what Decoder.forward adds first (:467).
__global__ __launch_bounds__(GTMS_WAVES * 64) void k_gtcn_ms(const float* __restrict__ xin, float* __restrict__ xout1,
                                                            float* __restrict__ xout2, const float* __restrict__ P,
                                                            int NB, float* __restrict__ state) {
    __shared__ __attribute__((aligned(16))) float sP[2 * GTCN_SIZE];
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long p = ((long)blockIdx.x * GTMS_WAVES + wave) * 16 + n;     // position on the flattened (stream, bin) axis
    const bool live = p < (long)NB * 33;
    const long pc = live ? p : 0;                                        // clamped: no select behind the loads
    const int sidx = (int)(pc / 33), ff = (int)(pc - (long)sidx * 33);
    float* st = state + (long)sidx * ST_FLOATS;
    const int tb = reinterpret_cast<const int*>(st)[0];
    // the history rows of a stack are requested up front; their latency hides behind the parameter copy / the
    // previous stack
    f32x4 t1[4], t2[4];
    int r2[4];
    auto fetch_rows = [&](const float* ring) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int d = 1 << k, m2d = 2 * d - 1, row0 = 2 * (d - 1);
            const int r1 = ((row0 + ((tb + d) & m2d)) * 33 + ff) * 16 + 4 * g;
            r2[k] = ((row0 + (tb & m2d)) * 33 + ff) * 16 + 4 * g;
            t1[k] = ld4(ring + r1);
            t2[k] = ld4(ring + r2[k]);
        }
    };
    fetch_rows(st + ST_G1_H);
    const f32x4 x0 = ld4(xin + pc * 16 + 4 * g);
    f32x4 x = x0;
    static_assert(GTCN_SIZE % 4 == 0 && P_GTCN % 4 == 0 && P_DEC % 4 == 0, "16-byte parameter copies");
    copy_params(sP, P, 2 * GTCN_SIZE, tid, GTMS_WAVES * 64);
    __syncthreads();
#pragma unroll
    for (int stack = 0; stack < 2; ++stack) {
        float* ring = st + (stack == 0 ? ST_G1_H : ST_G2_H);
        const float* pk = sP + stack * GTCN_SIZE;
        f32x4 a1[4], a2[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { a1[k] = t1[k]; a2[k] = t2[k]; }
        int q2[4] = {r2[0], r2[1], r2[2], r2[3]};
        if (stack == 0) fetch_rows(st + ST_G2_H);                        // the second stack's rows: in flight during the first
        tcn_block_ms<1>(x, pk + 0 * TCN_SIZE, a1[0], a2[0], ring + q2[0], live, n, g);
        tcn_block_ms<2>(x, pk + 1 * TCN_SIZE, a1[1], a2[1], ring + q2[1], live, n, g);
        tcn_block_ms<4>(x, pk + 2 * TCN_SIZE, a1[2], a2[2], ring + q2[2], live, n, g);
        tcn_block_ms<8>(x, pk + 3 * TCN_SIZE, a1[3], a2[3], ring + q2[3], live, n, g);
        if (live) st4((stack == 0 ? xout1 : xout2) + pc * 16 + 4 * g, stack == 0 ? x : x + x0);
    }
}

// ---------------------------------------------------------------------------- GTCN, offline form
// Same arithmetic, different ownership: wave w owns frequency bins 3w..3w+2 for ALL frames (11 waves x
// 3 bins = 33), a tile = 16 consecutive frames of one bin (lane n <-> frame t0+n).  The TCN couples
// positions only along time, so every tap of a wave's tile lies in that same wave's data: the y1
// history is a WAVE-PRIVATE LDS image per block and bin, [32 frame rows][16 slots], row = frame mod 32
// (the current chunk's 16 rows next to the previous chunk's).  A tap is one ds_read_b128 at
// "own row - d" (mod 32); nothing is shared between waves, so the chunk loop has NO barrier and the
// waves run decoupled.  (A register-only variant with DPP row rotations measured slower: a DPP
// rotate costs ~10 issue cycles on gfx950.)  Used when there is no stream state (offline forward);
// the ring form above serves streaming calls, where a chunk may hold a single frame.
constexpr int GB_LDS_P = 0;
constexpr int GB_RS = RS_WIDE;                                 // record pitch (conflict-free tile reads, see pl())
constexpr int GB_LDS_C = GB_LDS_P + GTCN_SIZE;                 // current chunk's y1: [33 bins][16 frames][GB_RS]
constexpr int GB_LDS_H = GB_LDS_C + 33 * 16 * GB_RS;           // history: block k: [33 bins][2d rows][GB_RS]
constexpr int GB_LDS_FLOATS = GB_LDS_H + 33 * 30 * GB_RS;
static_assert(GB_LDS_C % 4 == 0, "16B carve");
static_assert(GB_LDS_FLOATS * 4 <= 160 * 1024, "band GTCN LDS budget");

// cw: this wave's 3 tiles of the current-chunk image; hw: this wave's 3 bins of block D's history ring
// (row = frame mod 2d); n = lane's frame inside the chunk; t0 is a multiple of 16 >= 2d, so
// (t0 + n) mod 2d == n mod 2d.
// am1: the block's three PReLU slopes minus one, wave uniform and the same for every chunk (formed once, in k_gtcn_band).
template <int D, bool Q>
__device__ __forceinline__ void tcn_block_band(f32x4 (&x)[TPW], const float* pk, const float (&am1)[3], float* cw,
                                               float* hw, bool live, const Lane& L) {
    const int n = L.n, g = L.g;
    constexpr int M2D = 2 * D - 1, HR = 2 * D * GB_RS, RS = GB_RS;   // ring mask, floats per bin of the ring
    const float a1 = am1[0], a2 = am1[1], a3 = am1[2];
    f32x4 y1[TPW], acc[TPW];
    const long h_minus_c = hw - cw;
    // ring rows of the taps that lie before the chunk
    const int r1 = ((n - D) & M2D) * RS + 4 * g, r2 = (n & M2D) * RS + 4 * g;
    {
        const f32x4 A = ld4(pk + TCN_A1 + arow(n, g)), Bv = ld4(pk + TCN_B1 + 4 * g);
#pragma unroll
        for (int i = 0; i < TPW; ++i) acc[i] = Bv;
        mm16<TPW, Q>(A, x, acc);
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            y1[i] = rq<Q>(prelu4q<Q>(acc[i], a1));
            st4(cw + i * 16 * RS + n * RS + 4 * g, y1[i]);
        }
    }
    // the in-chunk taps were written by lanes of this wave: LDS operations of a wave complete in order,
    // only the compiler has to be kept from hoisting the reads above the writes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    {
        const f32x4 w0 = ld4(pk + TCN_DW + 4 * g), w1 = ld4(pk + TCN_DW + 16 + 4 * g),
                    w2 = ld4(pk + TCN_DW + 32 + 4 * g), B2 = ld4(pk + TCN_B2 + 4 * g);
        const f32x4 A = ld4(pk + TCN_A3 + arow(n, g)), B3 = ld4(pk + TCN_B3 + 4 * g);
        f32x4 y2[TPW];
        const int c1 = (n >= D ? n - D : n) * RS + 4 * g, c2 = (n >= 2 * D ? n - 2 * D : n) * RS + 4 * g;
        // one load per tap: the ADDRESS is chosen per lane (chunk image or ring; both sit in this wave's LDS), not the
        // data (two loads and four selects per tap)
        const int hc = (int)h_minus_c;
        const int b1 = n >= D ? c1 : hc + r1, s1 = n >= D ? 16 * RS : HR;
        const int b2 = n >= 2 * D ? c2 : hc + r2, s2 = n >= 2 * D ? 16 * RS : HR;
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const f32x4 p1 = ld4(cw + b1 + i * s1), p2 = ld4(cw + b2 + i * s2);
            y2[i] = rq<Q>(prelu4q<Q>(B2 + w0 * p2 + w1 * p1 + w2 * y1[i], a2));
            acc[i] = B3 + x[i];
        }
        mm16<TPW, Q>(A, y2, acc);
#pragma unroll
        for (int i = 0; i < TPW; ++i) x[i] = rq<Q>(prelu4q<Q>(acc[i], a3));
    }
    // ring update: the last 2d frames of the chunk (every live lane for the final, partial chunk is fine:
    // later frames overwrite earlier ones of the same row only in program order of a single lane set)
    if (live && n >= 16 - 2 * D) {
#pragma unroll
        for (int i = 0; i < TPW; ++i) st4(hw + i * HR + r2, y1[i]);
    }
}

// B, T: batch and row stride; gridDim.x workgroups share the (utterance, frame) axis (see span_begin); lens != nullptr
// (variable-length batch): one workgroup per utterance.
template <bool Q, bool SPANS = false>
__global__ __launch_bounds__(NTHR) void k_gtcn_band(const float* __restrict__ xin, float* __restrict__ xout,
                                                   const float* __restrict__ P, int B, int T,
                                                   const int* __restrict__ lens, const float* __restrict__ addend) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sP = smem + GB_LDS_P;
    float* sC = smem + GB_LDS_C;
    float* sHh = smem + GB_LDS_H;
    const Lane L = lane_info();
    const int tid = L.tid, n = L.n, g = L.g;
    SpanIter sit;
    #ifdef GT_EXP_SAMEUTT    // timing experiment only (wrong results): every workgroup works on one of eight utterances, so all
    int s_b = blockIdx.x & 7, s_fb = 0, s_wlo = 0, s_nT = T;   // hand-off traffic hits in L2: the kernels without HBM latency
#else
    int s_b = blockIdx.x, s_fb = 0, s_wlo = 0, s_nT = T;
#endif
    if constexpr (SPANS) {       // (`lens` is the PREFIX table of a variable-length batch here, see span_begin)
        if (!span_begin(sit, blockIdx.x, gridDim.x, B, T, lens)) return;
    } else {                     // one workgroup per utterance (lens: a variable-length batch, this utterance's frames)
        s_nT = lens ? min(T, 1 + (lens[blockIdx.x] >> 8)) : T;
    }
    copy_params(sP, P, GTCN_SIZE, tid, NTHR);
    for (int i = tid; i < 33 * 30 * GB_RS / 4; i += NTHR) st4(sHh + i * 4, splat(0.f));   // zero history (frames < 0)
    __syncthreads();
    using ht = typename HandOff<Q>::t;
    const int f0 = L.wave * TPW;                         // first bin of this wave
    float* cw = sC + f0 * 16 * GB_RS;
    // the PReLU slopes of the four blocks, minus one: twelve wave-uniform numbers that no chunk changes, kept in
    // scalar registers instead of being read from LDS and decremented in every block of every chunk.  (Not in the
    // SPANS form, whose span iterator leaves no room for them: it would spill, so it reads them per chunk.)
    auto slopes = [&](const float* pk, float (&a)[3]) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float v = slope_arg<Q>(pk[TCN_SLOPE + j]);
            a[j] = SPANS ? v : __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
        }
    };
    float am1[4][3];
    if constexpr (!SPANS) {
#pragma unroll
        for (int k = 0; k < 4; ++k) slopes(sP + k * TCN_SIZE, am1[k]);
    }
    for (int sg = 0;; ++sg) {
        if constexpr (SPANS) {
            if (!span_next(sit, B, T, lens, HALO_GTCN, s_b, s_fb, s_wlo, s_nT)) break;
        } else if (sg > 0) {
            break;
        }
        const long rb = (long)s_b * T + s_fb;            // first row of the segment in the hand-off tensors
        const ht* xinh = reinterpret_cast<const ht*>(xin) + rb * 528;
        ht* xouth = reinterpret_cast<ht*>(xout) + rb * 528;
        const ht* addh = addend ? reinterpret_cast<const ht*>(addend) + rb * 528 : nullptr;
        const int Ts = s_nT, wlo = SPANS ? s_wlo : 0;
        if (sg > 0) {
            // a second segment starts a new utterance: its history is zero again.  The rings are wave private (this
            // wave's three bins of every block), so no workgroup barrier: block k's slice is [3 bins][2d rows][GB_RS]
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int d2 = 2 << k, r0 = 2 * ((1 << k) - 1);
                float* hw = sHh + (33 * r0 + f0 * d2) * GB_RS;
                for (int i = L.lane; i < TPW * d2 * GB_RS / 4; i += 64) st4(hw + 4 * i, splat(0.f));
            }
            wave_lds_sync();
        }
        // the chunk's input is fetched one chunk ahead into registers (the waves run decoupled here, so an exposed
        // HBM latency at the top of every chunk is not hidden by a barrier wait elsewhere); the addend is only
        // needed at the store, so it is requested at the top of its own chunk.
        // Addresses: the three tensors are walked with one wave-uniform row counter (the chunk's first row, added to
        // the bases as a scalar) and ONE per-lane byte offset inside the chunk, (min(n, last live row) * 33 + f0) *
        // 16 + 4g records: a constant except in the final, partial chunk, where the rows past the end are clamped to
        // the last one (no select behind the loads).  The offset of chunk t0 + TC is formed when that chunk is
        // fetched and carried into the next trip, so a trip costs two vector instructions of address arithmetic.
        constexpr int EB = (int)sizeof(ht);
        const unsigned lane_off = (unsigned)(((f0 * 16 + 4 * g) * EB));
        auto chunk_off = [&](int t0f) -> unsigned {       // byte offset of the lane's record from row t0f of the segment
            return (unsigned)min(n, max(Ts - 1 - t0f, 0)) * (unsigned)(528 * EB) + lane_off;
        };
        auto row_ptr = [&](const ht* base, int t0f, unsigned off) {
            return reinterpret_cast<const ht*>(reinterpret_cast<const char*>(base + (long)t0f * 528) + off);
        };
        f32x4 xn[TPW];
        unsigned off_n = chunk_off(0);
#pragma unroll
        for (int i = 0; i < TPW; ++i) xn[i] = ldx<Q>(row_ptr(xinh, 0, off_n) + i * 16);
        for (int t0 = 0; t0 < Ts; t0 += TC) {
            const bool live = n < Ts - t0;
            const bool wr = live && n >= wlo - t0;             // warm-up frames of a segment are not stored
            const unsigned off = off_n;
            f32x4 x[TPW], ad[TPW];
#pragma unroll
            for (int i = 0; i < TPW; ++i) x[i] = xn[i];
            if (addend) {
#pragma unroll
                for (int i = 0; i < TPW; ++i) ad[i] = ldx<Q>(row_ptr(addh, t0, off) + i * 16);
            }
            // opaque offset: the block parameters are re-read from LDS every chunk; hoisting the four
            // blocks' fragments out of the chunk loop would need 128 registers and spill
            int po = 0;
            asm volatile("" : "+v"(po));
            if constexpr (SPANS) {
#pragma unroll
                for (int k = 0; k < 4; ++k) slopes(sP + po + k * TCN_SIZE, am1[k]);
            }
            // block k's ring: [33 bins][2d rows][16], blocks back to back (2, 4, 8, 16 rows per bin)
            tcn_block_band<1, Q>(x, sP + po + 0 * TCN_SIZE, am1[0], cw, sHh + (33 * 0 + f0 * 2) * GB_RS, live, L);
            // The next chunk is requested HERE, not at the top: the first block's residual is the last reader of this
            // chunk's input, so the loads land in the registers that held it and the loop carries xn without a copy
            // (requested at the top, xn -> x cost twelve moves a trip).  Three blocks remain to cover the latency.
            // Behind the last chunk it re-reads the segment's last row: the clamp keeps the address inside the
            // segment, and a load that is not conditional needs no second copy of xn either.
            const int t1 = t0 + TC < Ts ? t0 + TC : t0;
            off_n = chunk_off(t1);
#pragma unroll
            for (int i = 0; i < TPW; ++i) xn[i] = ldx<Q>(row_ptr(xinh, t1, off_n) + i * 16);
            tcn_block_band<2, Q>(x, sP + po + 1 * TCN_SIZE, am1[1], cw, sHh + (33 * 2 + f0 * 4) * GB_RS, live, L);
            tcn_block_band<4, Q>(x, sP + po + 2 * TCN_SIZE, am1[2], cw, sHh + (33 * 6 + f0 * 8) * GB_RS, live, L);
            tcn_block_band<8, Q>(x, sP + po + 3 * TCN_SIZE, am1[3], cw, sHh + (33 * 14 + f0 * 16) * GB_RS, live, L);
            ht* const o = const_cast<ht*>(row_ptr(xouth, t0, off));
            // one uniform branch around each form of the store: with a select per tile the compiler gave `ad` a value on
            // the path that has none (twelve moves a trip)
            if (addend) {
#pragma unroll
                for (int i = 0; i < TPW; ++i)
                    if (wr) stx<Q>(o + i * 16, rq<Q>(x[i] + ad[i]));
            } else {
#pragma unroll
                for (int i = 0; i < TPW; ++i)
                    if (wr) stx<Q>(o + i * 16, x[i]);
            }
        }
    }
}

// =============================================================================== decoder
// Decoder.forward (models/gtcrn_micro.py:464-469): x = de[i](x + en_outs[4-i]); three dense
// GTConvBlocks, de_convs.3 (ConvTranspose2d (1,5) stride (1,2), 33 -> 65) in gather form,
// de_convs.4 (16 -> 2, 65 -> 129, Tanh) in scatter form, then ERB.bs (:69-73), the complex
// ratio mask (:478-482) and the output permute (:529-530).
constexpr int DEC_Z_ROW = F1 + 2;                                 // Z rows carry a zero record at both ends
constexpr int DEC_ZS = 12;                                        // floats per Z record (10 live slots)
// parameters resident in LDS: the three blocks WITHOUT their dense matrices, then the de_convs.3/4 segment; the dense
// 3x3 of ONE block at a time sits in the stage buffer DN (the bf16 planes of all three would not fit: 45 KB), refilled
// from L2 while the previous block's TRALite runs
constexpr int DL_DE3M = 3 * GB_SIZE;                              // de_convs.3 matrices: 9 plane matrices (split) or the 5 fp32 ones
constexpr int DL_DE = DL_DE3M + DE3_16_MATS * 256;                // de_convs.3 bias / slope, de_convs.4: D_DE3_B .. D_BS_W
constexpr int DL_DN = DL_DE + (D_BS_W - D_DE3_B);                 // dense stage buffer
constexpr int DL_SIZE = DL_DN + DN16_SIZE;
// D_* offset -> LDS offset (the fp32 de_convs.3 matrices sit at DL_DE3M when the split form is off)
__device__ __forceinline__ constexpr int dl(int d_off) { return d_off >= D_DE3_B ? DL_DE + d_off - D_DE3_B : DL_DE3M + d_off - D_DE3_AE; }
static_assert(DL_DE % 4 == 0 && DL_DN % 4 == 0 && DN16_SIZE >= 9 * 256 && GBD_SIZE % 4 == 0 && D_DN16 % 4 == 0 &&
              D_DE3_16 % 4 == 0 && D_DE3_B == D_DE3_AE + 5 * 256, "16B carve");
// the decoder's parameter segment -> LDS (everything but the blocks' dense matrices, which go through the stage buffer)
template <bool SPLIT>
__device__ __forceinline__ void copy_dec_params(float* sP, const float* PF, int tid, int nthr) {
#pragma unroll
    for (int j = 0; j < 3; ++j) copy_params(sP + j * GB_SIZE, PF + P_DEC + D_BLK + j * GBD_SIZE, GB_SIZE, tid, nthr);
    if constexpr (SPLIT) copy_params(sP + DL_DE3M, PF + P_DEC + D_DE3_16, DE3_16_MATS * 256, tid, nthr);
    else copy_params(sP + DL_DE3M, PF + P_DEC + D_DE3_AE, 5 * 256, tid, nthr);
    copy_params(sP + DL_DE, PF + P_DEC + D_DE3_B, D_BS_W - D_DE3_B, tid, nthr);
}

// de_convs.3 = ConvTranspose2d(16,16,(1,5),stride (1,2)) in gather form for the wave's tiles: even output bin 2m takes
// taps k = 0, 2, 4 from input bins m+1, m, m-1, odd bin 2m+1 takes k = 1, 3 from m+1, m.  The input image (records of
// x, zero pad columns) is in LDS; rec0[i] = float offset of tile i's own record (slot group 0).
// SPLIT: on v_mfma_f32_16x16x32_bf16 like the dense 3x3 (x stored as three bf16 planes): K-chunk 0 = bins (m+1 | m)
// feeds the even AND the odd outputs (matrices E0, O0), K-chunk 1 = (m-1 | -) the even ones (E1): 18 instructions of
// 16 cycles instead of 20 of 32.  Otherwise: five fp32 slot matrices, the centre tap from the registers.
template <int TPW, bool SPLIT, bool Q, int RS>
__device__ __forceinline__ void de_conv3_tiles(const float* sW, const int (&rec0)[TPW], const f32x4 (&x)[TPW],
                                               const float* m3, const f32x4 Bv, int n, int g, f32x4 (&ae)[TPW],
                                               f32x4 (&ao)[TPW]) {
#pragma unroll
    for (int i = 0; i < TPW; ++i) { ae[i] = Bv; ao[i] = Bv; }
    if constexpr (SPLIT) {
        int gq = g;
        asm volatile("" : "+v"(gq));
        const bool second = gq >= 2;
        const int q16 = 4 * (gq & 1);
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            bf16x8 pe[3], po[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                pe[p] = *reinterpret_cast<const bf16x8*>(m3 + ((cc == 0 ? 0 : 2) * 3 + p) * 256 + arow(n, g));
                if (cc == 0) po[p] = *reinterpret_cast<const bf16x8*>(m3 + (1 * 3 + p) * 256 + arow(n, g));
            }
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                // chunk 0: lane groups g < 2 read bin m+1, g >= 2 bin m; chunk 1: g < 2 bin m-1, g >= 2 zero weights
                const int src = rec0[i] + (cc == 0 ? (second ? 0 : RS) : (second ? 0 : -RS)) + q16;
                bf16x8 bp[3];
#pragma unroll
                for (int p = 0; p < 3; ++p) bp[p] = *reinterpret_cast<const bf16x8*>(sW + src + 8 * p);
                ae[i] = split_mm6(pe, bp, ae[i]);
                if (cc == 0) ao[i] = split_mm6(po, bp, ao[i]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        const float* Ae = m3 + arow(n, g);
        const float* Ao = m3 + 3 * 256 + arow(n, g);
        // tap major over the three input bins f+1, f, f-1: the five slot matrices are read once per wave
        {
            const f32x4 A0 = ld4(Ae), A1 = ld4(Ao);
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                const f32x4 xp = ld4(sW + rec0[i] + 4 * g + RS);   // input bin f+1
                ae[i] = mm1<Q>(A0, xp, ae[i]);
                ao[i] = mm1<Q>(A1, xp, ao[i]);
            }
        }
        {
            const f32x4 A0 = ld4(Ae + 256), A1 = ld4(Ao + 256);
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                ae[i] = mm1<Q>(A0, x[i], ae[i]);
                ao[i] = mm1<Q>(A1, x[i], ao[i]);
            }
        }
        {
            const f32x4 A0 = ld4(Ae + 512);
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                const f32x4 xm = ld4(sW + rec0[i] + 4 * g - RS);   // input bin f-1
                ae[i] = mm1<Q>(A0, xm, ae[i]);
            }
        }
    }
}
template <int RW, int NS, bool MS>
struct DecLds {
    static constexpr int RS = RS_WIDE;                            // record pitch of the h image W (see pl(); split planes)
    static constexpr int RSS = 16;                                // ... of the v^2 image S
    static constexpr int P = 0;                                   // block parameters, de_convs.3/4, dense stage buffer
    static constexpr int I = P + DL_SIZE;                         // (the kernel-ready ERB.bs table has its own region, BS)
    static constexpr int H = I + 48;                              // ints: the three blocks' slot tables (I_DEC_BLK)
    static constexpr int EH = H + (MS ? NS * 3 * 2 * 35 * RS : 3 * RING_DENSE);
    static constexpr int TB = EH + NS * 48;                       // frame counter per row (ints; multi-stream mode)
    static constexpr int G = TB + 8;
    static constexpr int E = G + RW * 16 + RW * 8;                // (gates [RW][16] + y scratch [RW][8]); energies
    // region A: W + S during the blocks; afterwards Z, and behind it the mask m [2][RW][129] (+4: the 2-tap read of
    // the last bin) -- m is written after the last block has read S and is dead before the next chunk writes S
    static constexpr int A = E + (MS ? NS * 24 : (RW + 2) * 8);
    static constexpr int RWI = MS ? RW : RW + IMG_R0;             // image rows (two history rows in front of the chunk)
    // image row pitch in records: 41 where the LDS allows it (since round 3 the parameter region is 12 KB smaller): a
    // tile that runs over the end of a row continues 9 = 1 (mod 8) records further on and keeps the conflict-free
    // bank pattern (see EncLds); the multi-stream form has no room and stays at 35
    static constexpr int PT = MS ? 35 : 41;                       // (A/B on one box: 0.4138 vs 0.4157 ms at 35)
    static constexpr int S = A + RWI * PT * RS;
    static constexpr int ZSZ = RW * DEC_Z_ROW * DEC_ZS;
    static constexpr int M = A + ZSZ;
    static constexpr int MSZ = (2 * RW * F0 + 4 + 3) & ~3;
    static constexpr int AEND = (S + RW * 33 * RSS) > (M + MSZ) ? (S + RW * 33 * RSS) : (M + MSZ);
    static constexpr int BS = AEND;                               // per-bin ERB.bs table {first index, w0, w1, -}
    static constexpr int FLOATS = BS + NBINS * 4;
    static_assert(M % 4 == 0 && BS % 4 == 0 && D_BS_W % 4 == 0 && D_BS_TAB % 4 == 0 && S % 4 == 0 && DL_SIZE % 4 == 0, "16B carve");
    static_assert(FLOATS * 4 <= 160 * 1024, "decoder LDS budget");
    static_assert(DEC_SIZE % 4 == 0 && I % 4 == 0 && H % 4 == 0 && A % 4 == 0 && E % 4 == 0, "16B carve");
};
constexpr int DEC_LDS_FLOATS = DecLds<TC, 1, false>::FLOATS;
constexpr int DEC_MS_LDS_FLOATS = DecLds<MS_ROWS, MS_STREAMS, true>::FLOATS;

// DBG = true only for the stage-tap variant used by the parity tests (writes de0..de4 to `dbg`).
// MS: multi-stream single-frame mode, see k_encoder (NB = number of streams; the host remaps the strides).
// Q / qin / qout: the int8-weight / fp16-activation variant and its optional int8 boundary (see k_encoder); qout is
// the step of the output quantiser (y = (y_q - zero) * out_scale, tflite_infer.py:88-91).
// SPANS: see k_encoder
template <bool DBG, int TPW, bool MS, bool Q, bool SPANS = false>
__global__ __launch_bounds__(NTHR) void k_decoder(const float* __restrict__ xg, const float* __restrict__ en0,
                                                 const float* __restrict__ en1, const float* __restrict__ en2,
                                                 const float* __restrict__ en3, const float* __restrict__ en4,
                                                 const float* __restrict__ spec, long sb, long sf, long st,
                                                 float* __restrict__ out, long osb, long osf, long ost, int T,
                                                 const int* __restrict__ lens, int NB, float qin, float qout,
                                                 const float* __restrict__ PF, const int* __restrict__ PI,
                                                 float* __restrict__ state, float* __restrict__ dbg,
                                                 unsigned long long* __restrict__ stamps) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    STAMP_INIT(SS)
    constexpr int RW = MS ? MS_ROWS : TC;
    constexpr int NS = MS ? MS_STREAMS : 1;
    using LD = DecLds<RW, NS, MS>;
    float* sP = smem + LD::P;
    int* sI = reinterpret_cast<int*>(smem + LD::I);
    float* sH = smem + LD::H;
    float* sEH = smem + LD::EH;
    int* sTB = reinterpret_cast<int*>(smem + LD::TB);
    float* sG = smem + LD::G;
    constexpr int RS = LD::RS;
    float* sW = smem + LD::A;
    float* sS = smem + LD::S;
    float* sZ = smem + LD::A;
    constexpr int ZS = DEC_ZS;
    float* sM = smem + LD::M;
    float* sBS = smem + LD::BS;              // per-bin ERB.bs table {first index, w0, w1, -}, built by the host packer
    const Lane L = lane_info();
    const int tid = L.tid, n = L.n, g = L.g;
    // offline calls (no stream state, no per-utterance lengths): the workgroups share the (utterance, frame) axis, a share
    // is one or two segments (see span_begin); everything else: one workgroup per utterance / group of streams
    const int Tstride = T;
    static_assert(!SPANS || (!MS && !Q), "time spans: offline fp32 form");
    SpanIter sit;
    #ifdef GT_EXP_SAMEUTT    // timing experiment only (wrong results): every workgroup works on one of eight utterances, so all
    int s_b = blockIdx.x & 7, s_fb = 0, s_wlo = 0, s_nT = T;   // hand-off traffic hits in L2: the kernels without HBM latency
#else
    int s_b = blockIdx.x, s_fb = 0, s_wlo = 0, s_nT = T;
#endif
    if constexpr (SPANS) {     // (`lens` is the PREFIX table of a variable-length batch here, see span_begin)
        if (!span_begin(sit, blockIdx.x, gridDim.x, NB, T, lens)) return;
        span_next(sit, NB, Tstride, lens, HALO_BLOCKS, s_b, s_fb, s_wlo, s_nT);
    }
    int b = s_b;
    constexpr bool SPLIT = !Q && kSplitDense;
    // the dense 3x3 of block j -> the stage buffer by LDS-DMA (global_load_lds_dwordx4: 1 KB pieces, wave w moves pieces
    // w, w + 11; no registers are held while the data is in flight -- a register-staged copy spilled).  A DMA is a
    // pending LDS write on the vector-memory counter: gtconv_block's closing barrier (and the prologue's) waits for
    // vmcnt(0) in front of it; the first reader sits one more barrier later.
    // (Q && !MS: the fp16 K-chunk matrices the packer put at the head of the block's D_DN16 slot in the quantised buffer)
    constexpr bool HALFW = Q && !MS;
    constexpr int DN_PIECES = SPLIT ? DN16_SIZE / 256 : (HALFW ? DN16_CHUNKS : 9);
    auto dense_fetch = [&](int j) {
        const float* src = PF + P_DEC + ((SPLIT || HALFW) ? D_DN16 + j * DN16_SIZE : D_BLK + j * GBD_SIZE + GB_DN_A);
        int lz = L.lane;
        asm volatile("" : "+v"(lz));      // per-lane source addresses recomputed per call, not hoisted and kept live
        // (inline asm, not __builtin_amdgcn_global_load_lds: with the builtin the compiler treats every later LDS read as a
        // possible reader of the DMA and puts `s_waitcnt vmcnt(0)` in front of the next one -- which would also wait for
        // the en0 / next-chunk prefetches issued beside it, i.e. expose their HBM latency inside TRALite.  The stage
        // buffer has exactly one reader, two barriers away, behind the explicit vmcnt(0) of wg_barrier_vm().)
        for (int pi = L.wave; pi < DN_PIECES; pi += NW) {
            const float* gsrc = src + pi * 256 + 4 * lz;
            const unsigned lds_dst = (unsigned)(size_t)(__attribute__((address_space(3))) void*)(sP + DL_DN + pi * 256);
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep)
                         : "v"(gsrc), "s"(lds_dst)
                         : "memory");
        }
    };
    dense_fetch(0);
    constexpr bool SPLIT3 = SPLIT && kSplitDe3;     // de_convs.3 in the split form too
    copy_dec_params<SPLIT3>(sP, PF, tid, NTHR);
    if (tid < 48) sI[tid] = PI[I_DEC_BLK + tid];
    for (int f = tid; f < NBINS; f += NTHR) st4(sBS + f * 4, ld4(PF + P_DEC + D_BS_TAB + f * 4));
    if (tid < 4) sM[2 * RW * F0 + tid] = 0.f;
    float* stb = state ? state + (long)b * NS * ST_FLOATS : nullptr;    // first stream of this workgroup
    const int nlive = MS ? min(NS, NB - b * NS) : 1;
    int tbase = 0;
    if constexpr (MS) {
        rings_load_ms<NS, SPLIT ? RS_WIDE : 16>(sH, sEH, stb, ST_DEC_H, ST_DEC_E, nlive, tid);
        if (tid < 8) sTB[tid] = tid < nlive ? reinterpret_cast<const int*>(stb + (long)tid * ST_FLOATS)[0] : 0;
    } else {
        tbase = stb ? reinterpret_cast<const int*>(stb)[0] : 0;
        rings_load(sH, sEH, stb ? stb + ST_DEC_H : nullptr, stb ? stb + ST_DEC_E : nullptr, tbase, tid);
    }
    const Tiles<TPW> tt = make_tiles<TPW>(L);
    wg_barrier_vm();

    const long nbt = MS ? (long)gridDim.x * T : (long)NB * T;    // rows of a stage tensor (DBG taps)
    const float* const spec0 = spec;
    float* const out0 = out;
    const bool t_fast = st < sf;
    const int sf32 = (int)sf, st32 = (int)st, osf32 = (int)osf, ost32 = (int)ost;
    constexpr int MASK_ITEMS = (RW * NBINS + NTHR - 1) / NTHR;   // spectrogram bins per thread and chunk
    STAMP(SS, 0)

    // xg already holds gtcn2(x) + en_outs[4] (k_gtcn adds it on store).  Lanes past the end of the
    // utterance read a clamped, valid record (never stored), so no load sits behind a select and
    // every load's latency runs until its first use.
    // global addressing: wave-uniform chunk base pointers (SGPR pairs) + 32-bit per-lane offsets
    using ht = typename HandOff<Q>::t;
    // per segment: the first row of the hand-off tensors / spectrograms, the frame count T, the utterance-local index fb of
    // the first processed frame and the first local frame that is stored (wlo: the warm-up frames in front are not)
    long ob;
    // (the tensors' base pointers are kernel arguments, re-read from the argument segment where a row pointer is formed:
    // five pre-offset pointer pairs held across the chunk loop pushed the SPANS form into scalar-register spills)
    auto rowp = [&](const float* base, long rows, int rec) { return reinterpret_cast<const ht*>(base) + (ob + rows) * rec; };
    int wlo_v;
    auto seg_setup = [&](int sb_, int sfb, int swlo, int snT) {
        b = sb_;
        ob = (long)sb_ * Tstride + sfb;
        spec = spec0 + (long)sb_ * sb + (long)sfb * st;
        out = out0 + (long)sb_ * osb + (long)sfb * ost;
        T = snT;
        wlo_v = swlo;
    };
    seg_setup(s_b, s_fb, s_wlo, s_nT);
    if constexpr (!SPANS) {
        if (lens) T = min(T, 1 + (lens[b] >> 8));   // variable-length batch: from here on T = this utterance's frames
    }
    if constexpr (MS) T = nlive;                // one frame per live stream = nlive rows
    f32x4 xn[TPW];
segment_top:
    {
        const int np0 = min(RW, T) * 33;
        const ht* xg0 = rowp(xg, 0, 528);
#pragma unroll
        for (int i = 0; i < TPW; ++i) xn[i] = ldx<Q>(xg0 + (unsigned)((tt.pp(i) < np0 ? tt.pp(i) : 0) * 16 + 4 * g));
    }
    (void)en4;
    for (int t0 = 0; t0 < T; t0 += RW) {
        const int nfr = min(RW, T - t0), npos = nfr * 33;
        const int wlo = SPANS ? wlo_v : 0;      // first local frame that is stored (0 unless this is a warmed-up segment)
        f32x4 x[TPW];
#pragma unroll
        for (int i = 0; i < TPW; ++i) x[i] = xn[i];
        zero_row_pads<LD::RWI, RS, LD::PT>(sW, tid);  // region A was Z in the previous chunk (a barrier follows in the block)
        STAMP(SS, 1)
        // All 256 workgroups run in lock step, so a load burst right before its use is a chip-wide HBM
        // burst (25 MB at once costs ~10 k cycles).  The inputs of the tail are therefore requested
        // early and spread out: en_outs[0] after the last block's dense conv (two barrier intervals before
        // its use), the next chunk's x during the de_conv4 gather.
        f32x4 s0e[TPW], s0o[TPW];   // en_outs[0] for the even / odd output bins
        // ---- 3 x GTConvBlock (dense transposed 3x3); the last one is peeled so that s0e/s0o are live only
        //      from its hook on, not across the loop --------------------------------------------------------
        auto run_block = [&](int j, auto&& hook, auto vmk) {
            // the skip added to this block's output (en3, en2, en1; already in this stage's slot
            // order) is fetched up front so that its latency hides behind the block
            const ht* sk = rowp(j == 0 ? en3 : (j == 1 ? en2 : en1), t0, 528);
            f32x4 skv[TPW];
#pragma unroll
            for (int i = 0; i < TPW; ++i)
                skv[i] = ldx<Q>(sk + (unsigned)((tt.pp(i) < npos ? tt.pp(i) : 0) * 16 + 4 * g));
            BlockCtx c;
            c.pb = sP + j * GB_SIZE;
            c.gA = sP + DL_DN;
            c.ib = sI + j * 16;
            c.sW = sW; c.sHk = sH + j * RING_DENSE; c.sS = sS; c.sG = sG; c.sEHk = sEH + j * 16;
            c.sHtop = j == 0 ? sH : nullptr;          // region A was Z / m in the previous chunk
            c.sHnext = j < 2 ? sH + (j + 1) * RING_DENSE : nullptr;
            c.sE = smem + LD::E;
            c.sY = sG + RW * 16;
            c.nfr = nfr; c.tabs = tbase + t0;
            c.sTB = sTB;
            if constexpr (MS) {
                const int sidx = min(tt.tl[0], NS - 1);
                constexpr int RSM = SPLIT ? RS_WIDE : 16;      // record pitch of the LDS rings (rings_load_ms)
                c.ms_roff[0] = (int)(sH - sW) + sidx * (3 * 2 * 35 * RSM) + j * (2 * 35 * RSM);
                c.ms_tb[0] = sTB[sidx];
            } else {
                c.ms_roff[0] = 0; c.ms_tb[0] = 0;
            }
            // the next block's dense 3x3 (block 0 of the next chunk after the last one): the DMA starts once this block's
            // dense phase is over (the hook runs behind its closing barrier) and is waited for two barrier intervals
            // later, one barrier (the next block's point_conv1) before its first reader
            c.g_hist[0] = nullptr;
            gtconv_block<true, TPW, MS, Q, RS, LD::RSS, true, LD::PT, decltype(vmk)::value>(
                x, tt, c, L, [&] { dense_fetch(j == 2 ? 0 : j + 1); hook(); }, [] {} STAMP_ARG);
            if (DBG)
#pragma unroll
                for (int i = 0; i < TPW; ++i)
                    if (tt.pp(i) < npos && t0 + tt.tl[i] >= wlo)
                        st4(dbg + ((long)j * nbt + ob + t0) * 528 + tt.pp(i) * 16 + 4 * g, x[i]);
#pragma unroll
            for (int i = 0; i < TPW; ++i) x[i] = rq<Q>(x[i] + skv[i]);
            STAMP(SS, 8)
        };
#pragma unroll 1
        for (int j = 0; j < 2; ++j) run_block(j, [] {}, std::integral_constant<int, 0>{});
        run_block(2, [&] {
            const ht* en0c = rowp(en0, t0, F1 * 16);
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                // record of output bin 2f (even) and 2f+1 (odd; for f = 32 the clamped record is unused)
                const unsigned o0 = (unsigned)((tt.pp(i) < npos ? tt.tl[i] * F1 + 2 * tt.ff[i] : 0) * 16 + 4 * g);
                s0e[i] = ldx<Q>(en0c + o0);
                s0o[i] = ldx<Q>(en0c + o0 + (tt.ff[i] < 32 ? 16u : 0u));
            }
        }, std::integral_constant<int, 2 * TPW>{});
        // ---- de_convs.3: gather form; input image in sW rows (pad columns are zero).  Every wave is
        // past the last block's tap reads (they precede that block's 2nd barrier), so sW is free.
        int rec3[TPW];
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            rec3[i] = o35<RS, LD::RWI - RW, LD::PT>(tt, i, 0);
            if constexpr (SPLIT3) st_split(sW, rec3[i], g, x[i]);
            else st4(sW + rec3[i] + 4 * g, x[i]);
        }
        STAMP(SS, 9)
        wg_barrier();
        STAMP(SS, 10)
        f32x4 ze[TPW], zo[TPW];
        {
            const f32x4 Bv = ld4(sP + dl(D_DE3_B) + 4 * g);
            const float a = slope_arg<Q>(sP[dl(D_DE3_S)]);
            f32x4 ae[TPW], ao[TPW];
            de_conv3_tiles<TPW, SPLIT3, Q, RS>(sW, rec3, x, sP + DL_DE3M, Bv, n, g, ae, ao);
            const f32x4 A4 = ld4(sP + dl(D_DE4_A) + arow(n, g));
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                f32x4 e2 = rq<Q>(prelu4q<Q>(ae[i], a)), o2 = rq<Q>(prelu4q<Q>(ao[i], a));
                if (DBG && tt.pp(i) < npos && t0 + tt.tl[i] >= wlo) {
                    float* d3 = dbg + 3 * nbt * 528 + ((ob + t0 + tt.tl[i]) * F1) * 16 + 4 * g;
                    st4(d3 + (2 * tt.ff[i]) * 16, e2);
                    if (tt.ff[i] < 32) st4(d3 + (2 * tt.ff[i] + 1) * 16, o2);
                }
                // + en_outs[0] (identity slot order), then de_convs.4 in scatter form
                e2 = rq<Q>(e2 + s0e[i]);
                o2 = rq<Q>(o2 + s0o[i]);
                ze[i] = mm1<Q>(A4, e2, splat(0.f));
                zo[i] = mm1<Q>(A4, o2, splat(0.f));
            }
        }
        wg_barrier();  // all taps of sW read: region A becomes Z[tl][65][16]
        STAMP(SS, 11)
        // Z records hold the 10 live rows of the de_convs.4 slot matrix (+2 zero ones): 12 floats, written by the slot
        // groups g < 3.  The 48-byte pitch spreads the records over the banks (the de_convs.4 gather below reads them
        // with 4-byte loads: a 64-byte pitch put 32 lanes on four banks)
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            if (g < 3) {
                st4(sZ + (tt.tl[i] * DEC_Z_ROW + 1 + 2 * tt.ff[i]) * ZS + 4 * g, ze[i]);
                if (tt.ff[i] < 32) st4(sZ + (tt.tl[i] * DEC_Z_ROW + 2 + 2 * tt.ff[i]) * ZS + 4 * g, zo[i]);
            }
        }
        {   // zero records at both ends of every Z row (region A held W / S)
            int tz = tid;
            asm volatile("" : "+v"(tz));
            if (tz < RW * 2 * 4 && (tz & 3) < 3) {
                float z = 0.f;
                asm volatile("" : "+v"(z));
                st4(sZ + ((tz >> 3) * DEC_Z_ROW + ((tz >> 2) & 1) * (DEC_Z_ROW - 1)) * ZS + 4 * (tz & 3), splat(z));
            }
        }
        // the input spectrogram for the mask is fetched here so that its latency hides behind the
        // de_convs.4 gather below
        float2 spv[MASK_ITEMS];
        {
            // item coordinates recomputed per chunk (opaque tid): hoisted out of the chunk loop they would be
            // spilled, and every scratch reload drains the loads in flight (scratch shares vmcnt)
            int tz = tid;
            asm volatile("" : "+v"(tz));
            int tq, f;
            spec_item_first(tz, t_fast, tq, f);
            const float* sbase = spec + (long)t0 * st;       // wave-uniform; per-lane offsets fit in 31 bits (api.cpp)
#pragma unroll
            for (int q = 0; q < MASK_ITEMS; ++q) {
                const bool ok = tq < nfr && f < NBINS;
                spv[q] = *reinterpret_cast<const float2*>(sbase + (ok ? f * sf32 + tq * st32 : 0));
                spec_item_next(t_fast, tq, f);
            }
        }
        STAMP(SS, 15)
        wg_barrier();
        STAMP(SS, 12)
        // next chunk's input: x is dead, so its registers are reused for the prefetch
        if (t0 + RW < T) {
            const int npn = min(RW, T - t0 - RW) * 33;
            const ht* xgn = rowp(xg, t0 + RW, 528);
#pragma unroll
            for (int i = 0; i < TPW; ++i) xn[i] = ldx<Q>(xgn + (unsigned)((tt.pp(i) < npn ? tt.pp(i) : 0) * 16 + 4 * g));
        }
        // de_convs.4 gather + BN + Tanh: m[o][f''] = tanh(b[o] + sum_k z[(f''+2-k)/2][o*5+k]).  Branch free:
        // even f'' = 2m takes k = 0,2,4 from rows m+1, m, m-1; odd f'' = 2m+1 takes k = 1,3 from rows m+1, m
        // and a zero slot (rows 10..15 of the de_conv4 slot matrix are zero); the end records are zero.
        // Thread <-> (frame parity h, output channel o, bin f'') for the whole chunk, the RW / 2 frames of that parity in
        // an unrolled loop: everything that depends on (o, f'') is computed once per chunk and the per-frame addresses
        // are immediate offsets (an item loop over the flattened index spent ~50 vector instructions per element on
        // index arithmetic).  Frames past a short last chunk are computed from stale rows and never read.
        {
            static_assert(4 * F0 <= NTHR && RW % 2 == 0, "two threads per (o, f'')");
            int tz = tid;
            asm volatile("" : "+v"(tz));
            if (tz < 4 * F0) {
                const int h = tz >= 2 * F0 ? 1 : 0, c = tz - h * 2 * F0, o = c >= F0 ? 1 : 0, fq = c - o * F0;
                const int par = fq & 1, m = fq >> 1;
                const float* zr = sZ + (h * DEC_Z_ROW + 1 + m) * ZS;
                const float* r1 = zr + ZS + o * 5 + par;
                const float* r2 = zr + o * 5 + 2 + par;
                const float* r3 = zr - ZS + (par ? 10 : o * 5 + 4);
                const float bias = sP[dl(D_DE4_B) + o];
                float* mo = sM + (o * RW + h) * F0 + fq;
#pragma unroll
                for (int j = 0; j < RW / 2; ++j) {
                    constexpr int ZF = 2 * DEC_Z_ROW * ZS;          // floats between frames t and t + 2
                    const float sum = bias + r1[j * ZF] + r2[j * ZF] + r3[j * ZF];
                    mo[j * 2 * F0] = rq1<Q>(fast_tanh(sum));
                }
            }
        }
        wg_barrier();
        STAMP(SS, 13)
        if (DBG)
            for (int idx = tid; idx < 2 * nfr * F0; idx += NTHR) {
                const int fq = idx % F0, ot = idx / F0, o = ot >= nfr ? 1 : 0, tq = ot - o * nfr;
                if (t0 + tq >= wlo)
                    dbg[3 * nbt * 528 + nbt * F1 * 16 + (((long)b * 2 + o) * Tstride + (ob - (long)b * Tstride) + t0 + tq) * F0 + fq] =
                        sM[(o * RW + tq) * F0 + fq];
            }
        // ---- ERB.bs + complex ratio mask + output layout --------------------------------------------
        {
            int tz = tid;
            asm volatile("" : "+v"(tz));
            int tq, f;
            spec_item_first(tz, t_fast, tq, f);
            float* obase = out + (long)t0 * ost;
            // items in groups of three: the table rows of a group are requested together, then its twelve mask values,
            // then the arithmetic and the (predicated) stores -- one LDS round trip per stage and group instead of two
            // per item (an item behind its own `if` is a basic block of its own: nothing of the next item was issued
            // before the previous one had finished).  Out-of-range items read item 0's (valid) entries.
            constexpr int GRP = 3;
            static_assert(MASK_ITEMS % GRP == 0, "mask items come in groups of three");
#pragma unroll
            for (int q0 = 0; q0 < MASK_ITEMS; q0 += GRP) {
                bool ok[GRP], wr[GRP];
                int fo[GRP];
                const float* m0[GRP];
                f32x4 tb[GRP];
#pragma unroll
                for (int j = 0; j < GRP; ++j) {
                    ok[j] = tq < nfr && f < NBINS;
                    wr[j] = ok[j] && t0 + tq >= wlo;       // warm-up frames of a segment are not stored
                    const int fc = ok[j] ? f : 0, tc = ok[j] ? tq : 0;
                    tb[j] = ld4(sBS + fc * 4);
                    m0[j] = sM + tc * F0;
                    fo[j] = f * osf32 + tq * ost32;
                    spec_item_next(t_fast, tq, f);
                }
                float a0[GRP], a1[GRP], b0[GRP], b1[GRP];
#pragma unroll
                for (int j = 0; j < GRP; ++j) {
                    const float* mp = m0[j] + __float_as_int(tb[j][0]);
                    a0[j] = mp[0]; a1[j] = mp[1]; b0[j] = mp[RW * F0]; b1[j] = mp[RW * F0 + 1];
                }
#pragma unroll
                for (int j = 0; j < GRP; ++j) {
                    // second tap selected, not multiplied by a zero weight: for the last band it would read the
                    // first element of the next frame's row, which may be stale (0 * NaN)
                    const bool two = tb[j][2] != 0.f;
                    const float mr = rq1<Q>(tb[j][1] * a0[j] + (two ? tb[j][2] * a1[j] : 0.f));
                    const float mi = rq1<Q>(tb[j][1] * b0[j] + (two ? tb[j][2] * b1[j] : 0.f));
                    float re = spv[q0 + j].x, im = spv[q0 + j].y;
                    if constexpr (Q) {
                        if (qin > 0.f) {       // the mask multiplies the model's own (boundary-quantised) input
                            re = fminf(fmaxf(rintf(re / qin), -128.f), 127.f) * qin;
                            im = fminf(fmaxf(rintf(im / qin), -128.f), 127.f) * qin;
                        }
                        re = rq1<Q>(re);
                        im = rq1<Q>(im);
                    }
                    float yr = rq1<Q>(re * mr - im * mi), yi = rq1<Q>(im * mr + re * mi);
                    if constexpr (Q) {
                        if (qout > 0.f) {
                            yr = fminf(fmaxf(rintf(yr / qout), -128.f), 127.f) * qout;
                            yi = fminf(fmaxf(rintf(yi / qout), -128.f), 127.f) * qout;
                        }
                    }
                    if (wr[j]) *reinterpret_cast<float2*>(obase + fo[j]) = make_float2(yr, yi);
                }
            }
        }
        wg_barrier();  // sM and region A are rewritten by the next chunk
        STAMP(SS, 14)
    }
    if constexpr (SPANS) {
        if (span_next(sit, NB, Tstride, lens, HALO_BLOCKS, s_b, s_fb, s_wlo, s_nT)) {
            // the share runs on into the next utterance: zero history again (every wave is behind the barrier that closed
            // the last chunk), then the same chunk loop; block 0 copies its (zero) history into the image itself
            rings_load(sH, sEH, nullptr, nullptr, 0, tid);
            wg_barrier();
            seg_setup(s_b, s_fb, s_wlo, s_nT);
            goto segment_top;
        }
    }
    STAMP_OUT(SS, stamps)
    if (stb) {
        wg_barrier();
        if constexpr (MS) {
            rings_store_ms<NS, SPLIT ? RS_WIDE : 16>(sH, sEH, stb, ST_DEC_H, ST_DEC_E, nlive, tid);
            if (tid < nlive) reinterpret_cast<int*>(stb + (long)tid * ST_FLOATS)[0] = (sTB[tid] + 1) & 0xFFFF;
        } else {
            rings_store(sH, sEH, stb + ST_DEC_H, stb + ST_DEC_E, tbase + T, tid);
            if (tid == 0) reinterpret_cast<int*>(stb)[0] = (tbase + T) & 0xFFFF;  // frame counter (rings use mod 16)
        }
    }
}

// =============================================================================== streaming step, ONE launch
// StreamGTCRNMicro.forward for N streams x one new frame (gtcrn_micro_stream.py:541-574, the loop :626-635) as a
// SINGLE kernel: in multi-stream mode a workgroup's four streams never leave it between encoder, GTCN and decoder, so
// the three launches of that step (k_encoder<MS> -> k_gtcn_ms -> k_decoder<MS>) collapse into one:
//   * one prologue: every parameter segment (encoder 19 KB, both GTCN stacks 20 KB, decoder 31 KB incl. the stage
//     buffer of one block's dense planes) is resident in LDS for the whole step;
//   * nothing is handed over through HBM: en4 -> GTCN -> decoder stay in registers (the MS tile geometry and
//     k_gtcn_ms's flattened (stream, bin) positions are the same mapping), the skips en1..en3 stay in registers in
//     their consumer's slot order, en0 stays in LDS;
//   * the h history of a GTConv block is NOT a resident ring set any more (4 streams x 3 blocks x 2 rows: 54 KB fp32 for
//     the encoder, 81 KB split for the decoder): it is a per-block LDS image of the two old rows, fetched from the
//     stream state one block ahead (two 16-byte loads per thread) and written while the previous block's TRALite
//     runs; the ONE new row goes straight from the registers to the state (gtconv_block, g_hist).  State traffic per
//     block and stream: 2 rows read, 1 row written -- what SURVEY 8d's 94 KB bound counts;
//   * every global load of a later phase is requested a phase or more ahead (GTCN rows during the last encoder block,
//     decoder history during the GTCN, dense planes by LDS-DMA during the previous block).
// Same helper code (gtconv_block, tcn_block_ms, the front-end expressions) as the three-launch form, same rounding:
// streamed == offline bit for bit (tests/test_gpu_stream.py).  The three-launch form remains for the stage taps.
// Launches of many rounds of workgroups: every workgroup walks the same phases, all 256 CUs start together, and the phases
// that request the GTCN history rows (a third of the step's state traffic within a fifth of its time) then ask for more
// than the HBM delivers -- the per-block stamps of the GTCN phase show the LATER blocks of the first stack waiting for rows
// that were requested with the first block's (profiles/r06_ab_stream_wide.txt).  The first round's workgroups therefore
// start one of 32 phase shifts late (a sleep, once per launch); every CU runs its workgroups back to back, so the
// shift persists and the chip-wide demand is spread over the step.  `unit` = 0: no stagger (launches of a few rounds).
__device__ __forceinline__ void stagger_start(int unit) {
#ifndef GT_EXP_NOSTAGGER
    // unit: low byte = sleeps of 8 x 64 clocks per phase shift, the bits above = number of phase shifts (a power of two <= 256)
    if (unit > 0 && blockIdx.x < 256) {
        // (consecutive workgroups go to consecutive XCDs: the shifts are spread inside every XCD first)
        const int ph = ((blockIdx.x >> 3) + 32 * (blockIdx.x & 7)) & ((unit >> 8) - 1);
        for (int i = 0; i < ph * (unit & 255); ++i) __builtin_amdgcn_s_sleep(8);
    }
#endif
}
struct SmLds {
    static constexpr int RW = MS_ROWS, NS = MS_STREAMS;
    static constexpr int PE = 0;                                  // encoder segment, then both GTCN stacks (contiguous in PF too)
    static constexpr int PG = PE + ENC_SIZE;
    static constexpr int PD = PG + 2 * GTCN_SIZE;                 // decoder: DL_* layout (blocks, de_convs, dense stage buffer)
    static constexpr int I = PD + DL_SIZE;                        // ints: the tables without the ERB.bs index ranges
    static constexpr int BS = I + ((P_INTS - ENC_I_SKIP + 3) & ~3);
    static constexpr int EHE = BS + NBINS * 4;                    // energy rings [NS][3][2][8], encoder / decoder
    static constexpr int EHD = EHE + NS * 48;
    static constexpr int TB = EHD + NS * 48;
    static constexpr int G = TB + 8;
    static constexpr int E = G + RW * 16 + RW * 8;
    static constexpr int EN0 = E + NS * 24;                       // en0 of the step [NS][65][16] (the decoder tail adds it)
    static constexpr int X = EN0 + NS * F1 * 16;                  // ---- region shared by the encoder and decoder phases
    static constexpr int HE = X;                                  // encoder: history image [NS][2][35][16]
    static constexpr int A = HE + NS * 2 * 35 * 16;               //          staged spectrogram, then E0, then W + S
    static constexpr int B = A + RW * ENC_E0_ROW * 16;            //          EB + F0
    static constexpr int SE = A + RW * 35 * 16;
    static constexpr int ENC_END = B + 3 * RW * EB_ROW + 3 * RW * F0_ROW;
    static constexpr int RSD = RS_WIDE;                           // decoder: 96-byte records (split planes)
    static constexpr int HD = X;                                  //          history image [NS][2][35][24]
    static constexpr int W = HD + NS * 2 * 35 * RSD;
    static constexpr int SD = W + RW * 35 * RSD;
    static constexpr int ZSZ = RW * DEC_Z_ROW * DEC_ZS;
    static constexpr int M = W + ZSZ;
    static constexpr int MSZ = (2 * RW * F0 + 4 + 3) & ~3;
    static constexpr int DEC_END = (SD + RW * 33 * 16) > (M + MSZ) ? (SD + RW * 33 * 16) : (M + MSZ);
    static constexpr int FLOATS = ENC_END > DEC_END ? ENC_END : DEC_END;
    static_assert(FLOATS * 4 <= 160 * 1024, "fused streaming step: LDS budget");
    static_assert(SE + RW * 33 * 16 <= ENC_END && 3 * RW * NBINS <= RW * ENC_E0_ROW * 16, "encoder overlay");
    static_assert(PG % 4 == 0 && PD % 4 == 0 && I % 4 == 0 && BS % 4 == 0 && EHE % 4 == 0 && G % 4 == 0 && E % 4 == 0 &&
                  EN0 % 4 == 0 && X % 4 == 0 && A % 4 == 0 && B % 4 == 0 && W % 4 == 0 && SD % 4 == 0 && M % 4 == 0, "16B carve");
};
constexpr int SM_LDS_FLOATS = SmLds::FLOATS;

// (diagnostic build: phase stamps 0 prologue .. first barrier, 1 ERB bands, 2 SFE, 3 en_conv0, 4 en_conv1; encoder blocks
// 10 pc1 / 11 depth + pc2 / 12 TRALite, 8 after a block; 9 both GTCN stacks; 13 decoder set-up; decoder blocks 5 / 6 / 7;
// 14 de_convs.3/4 .. tanh, 15 mask + epilogue)
// (the body: stream_ms_body.inc, shared with k_stream_ms_slots)
#define SROW(sidx) (IDX ? (long)sSlot[sidx] * ST_FLOATS : (long)(sidx) * ST_FLOATS)     // (sSlot is volatile: read per use)
__global__ __launch_bounds__(NTHR) void k_stream_ms(const float* __restrict__ spec, long sb, long sf,
                                                   float* __restrict__ out, long osb, long osf, int NB,
                                                   const float* __restrict__ PF, const int* __restrict__ PI,
                                                   float* __restrict__ state, unsigned long long* __restrict__ stamps,
                                                   int stagger) {
    [[maybe_unused]] const int* const slots = nullptr;
    [[maybe_unused]] const int* const cnt = nullptr;
#define GT_SM_IDX false
#include "stream_ms_body.inc"
#undef GT_SM_IDX
}
// the indexed form: NB = max_active sizes the grid, cnt (device, may be null: NB) says how many rows step, slots names
// their states
__global__ __launch_bounds__(NTHR) void k_stream_ms_slots(const float* __restrict__ spec, long sb, long sf,
                                                         float* __restrict__ out, long osb, long osf, int NB,
                                                         const float* __restrict__ PF, const int* __restrict__ PI,
                                                         float* __restrict__ state, unsigned long long* __restrict__ stamps,
                                                         int stagger, const int* __restrict__ slots,
                                                         const int* __restrict__ cnt) {
#define GT_SM_IDX true
#include "stream_ms_body.inc"
#undef GT_SM_IDX
}
#undef STL

// =============================================================================== streaming step, ONE launch, WIDE form
// The same step as k_stream_ms for SEVEN streams per workgroup.  k_stream_ms is a chain of ~35 barrier-delimited phases
// whose length hardly depends on the number of streams (65 k cycles for one stream, 75 k for four: profiles/
// r04_phase_profile_stream.txt), so the lever for capacity (N >> 1024 streams per GPU) is more streams per workgroup;
// what stood in the way was LDS: 86 KB of resident parameters.  Here:
//   * eight waves x TWO tiles: 16 tiles = 256 positions for 7 x 33 = 231 (90 % of the lanes live; the 11 x 1 form: 75 %),
//     two independent MFMA chains per wave, 256 VGPRs per wave;
//   * the parameters are STREAMED, each segment by LDS-DMA a phase or more before its first reader:
//       P1   encoder front end + blocks (19 KB)  -> after the encoder: decoder blocks, de_convs.3/4 (20 KB, same slot)
//       GP   both GTCN stacks (19.6 KB)          -> into the dead EB / F0 region of the encoder front end, during the blocks
//       DN   one decoder block's dense planes (15 KB), as in k_stream_ms;   BS  the ERB.bs table (4 KB)
//     40 KB instead of 86 KB, which is what lets seven streams' images (en0, history, W / S / Z / M) fit in 160 KB;
//   * images carry exactly NS rows; the nine lanes past position 231 (and the whole last tile) compute on whatever they
//     read and store nothing (gtconv_block PMAX).
// Same helper code and source expressions as k_stream_ms and the three-launch form: bit-identical outputs and state
// (tests/test_gpu_stream.py).  Chosen by launch_stream_step for stream counts that fill the chip more than once.
struct SwCfg {
    static constexpr int NWV = 8, NT = NWV * 64, TPW = 2, NS = 7, RW = 7, RWG = 8, PMAX = NS * 33;
    static_assert(NWV * TPW * 16 >= PMAX && RWG * 33 >= NWV * TPW * 16, "tiles cover the streams; gate rows cover the tiles");
};
template <class CF>
struct SwLds {
    static constexpr int RW = CF::RW, NS = CF::NS;
    static constexpr bool SPLIT = kSplitDense;
    static constexpr int P1SZ = ((ENC_SIZE > DL_DN ? ENC_SIZE : DL_DN) + 3) & ~3;
    static constexpr int P1 = 0;                                  // encoder segment, later the decoder's DL_* layout up to DL_DN
    static constexpr int DN = P1 + P1SZ;                          // dense stage buffer
    static constexpr int BS = DN + (SPLIT ? DN16_SIZE : 9 * 256);
    static constexpr int I = BS + NBINS * 4;
    static constexpr int EHE = I + ((P_INTS - ENC_I_SKIP + 3) & ~3);
    static constexpr int EHD = EHE + NS * 48;
    static constexpr int TB = EHD + NS * 48;
    static constexpr int G = TB + 8;
    static constexpr int E = G + CF::RWG * 16 + CF::RWG * 8;
    static constexpr int EN0 = E + ((NS * 24 + 3) & ~3);
    static constexpr int X = EN0 + NS * F1 * 16;                  // ---- region shared by the encoder, GTCN and decoder phases
    static constexpr int HE = X;                                  // encoder: history image [NS][2][35][16]
    static constexpr int A = HE + NS * 2 * 35 * 16;               //          staged spectrogram, then E0, then W + S (both inside A)
    static constexpr int SE = A + RW * 35 * 16;
    static constexpr int B = A + RW * ENC_E0_ROW * 16;            //          EB + F0; from the first block on: the GTCN parameters
    static constexpr int BSZ = (3 * RW * EB_ROW + 3 * RW * F0_ROW + 3) & ~3;
    static constexpr int GP = B;
    static constexpr int ENC_END = B + BSZ;
    static constexpr int RSD = RS_WIDE;                           // decoder: 96-byte records (split planes)
    static constexpr int HD = X;                                  //          history image [NS][2][35][24]
    static constexpr int W = HD + NS * 2 * 35 * RSD;
    static constexpr int SD = W + RW * 35 * RSD;
    static constexpr int ZSZ = RW * DEC_Z_ROW * DEC_ZS;
    static constexpr int M = W + ZSZ;
    static constexpr int MSZ = (2 * RW * F0 + 4 + 3) & ~3;
    static constexpr int DEC_END = (SD + RW * 33 * 16) > (M + MSZ) ? (SD + RW * 33 * 16) : (M + MSZ);
    static constexpr int FLOATS = ENC_END > DEC_END ? ENC_END : DEC_END;
    static_assert(FLOATS * 4 <= 160 * 1024, "wide streaming step: LDS budget");
    static_assert(SE + RW * 33 * 16 <= B && 3 * RW * NBINS <= RW * ENC_E0_ROW * 16, "encoder overlay: W + S inside the E0 region");
    static_assert(2 * GTCN_SIZE <= BSZ, "the GTCN parameters fit the EB / F0 region");
    static_assert(CF::NWV * 320 <= RW * 33 * 16 && CF::NWV * 320 <= BSZ, "wave-private permutation scratch");
    static_assert(DN % 4 == 0 && BS % 4 == 0 && I % 4 == 0 && EHE % 4 == 0 && G % 4 == 0 && E % 4 == 0 && EN0 % 4 == 0 &&
                  X % 4 == 0 && A % 4 == 0 && B % 4 == 0 && SE % 4 == 0 && W % 4 == 0 && SD % 4 == 0 && M % 4 == 0, "16B carve");
};
constexpr int SW_LDS_FLOATS = SwLds<SwCfg>::FLOATS;

template <int D, int N>
__device__ __forceinline__ void tcn_block_msn(f32x4 (&x)[N], const float* pk, const f32x4 (&t1)[N], const f32x4 (&t2)[N],
                                              float* const (&ring_r2)[N], const bool (&live)[N], int n, int g) {
    // (tcn_block_ms for N tiles of a wave: the same expressions per tile, the tiles' MFMA chains interleaved)
    const float a1 = pk[TCN_SLOPE] - 1.0f, a2 = pk[TCN_SLOPE + 1] - 1.0f, a3 = pk[TCN_SLOPE + 2] - 1.0f;
    f32x4 y1[N], acc[N];
    {
        const f32x4 A = ld4(pk + TCN_A1 + arow(n, g)), Bv = ld4(pk + TCN_B1 + 4 * g);
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] = Bv;
        mm16<N>(A, x, acc);
#pragma unroll
        for (int i = 0; i < N; ++i) y1[i] = prelu4(acc[i], a1);
    }
    {
        const f32x4 w0 = ld4(pk + TCN_DW + 4 * g), w1 = ld4(pk + TCN_DW + 16 + 4 * g),
                    w2 = ld4(pk + TCN_DW + 32 + 4 * g), B2 = ld4(pk + TCN_B2 + 4 * g);
        const f32x4 A = ld4(pk + TCN_A3 + arow(n, g)), B3 = ld4(pk + TCN_B3 + 4 * g);
        f32x4 y2[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            y2[i] = prelu4(B2 + w0 * t2[i] + w1 * t1[i] + w2 * y1[i], a2);
            acc[i] = B3 + x[i];
        }
        mm16<N>(A, y2, acc);
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = prelu4(acc[i], a3);
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
        if (live[i]) st4(ring_r2[i], y1[i]);
}

template <class CF, bool IDX = false>
__global__ __launch_bounds__(CF::NT) void k_stream_wide(const float* __restrict__ spec, long sb, long sf,
                                                       float* __restrict__ out, long osb, long osf, int NB,
                                                       const float* __restrict__ PF, const int* __restrict__ PI,
                                                       float* __restrict__ state, unsigned long long* __restrict__ stamps,
                                                       int stagger, const int* __restrict__ slots,
                                                       const int* __restrict__ cnt) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if constexpr (IDX) {
        NB = slot_count(cnt, NB);
        if (NB - (int)blockIdx.x * CF::NS <= 0) {                 // (workgroup uniform; nothing issued, no barrier met)
            STAMP_ZERO(stamps)
            return;
        }
    }
    stagger_start(stagger);
    STAMP_INIT(SS)
    using LD = SwLds<CF>;
    constexpr int RW = CF::RW, NS = CF::NS, NWV = CF::NWV, NT = CF::NT, TPW = CF::TPW, PMAX = CF::PMAX;
    constexpr bool SPLIT = kSplitDense;
    constexpr bool SPLIT3 = SPLIT && kSplitDe3;
    float* sP1 = smem + LD::P1;
    float* sPE = sP1;                                              // P1 while the encoder runs ...
    float* sPD = sP1;                                              // ... and from the GTCN on (DL_* offsets below DL_DN)
    float* sDN = smem + LD::DN;
    float* sPG = smem + LD::GP;
    int* sI = reinterpret_cast<int*>(smem + LD::I);
    float* sBS = smem + LD::BS;
    float* sEHe = smem + LD::EHE;
    float* sEHd = smem + LD::EHD;
    int* sTB = reinterpret_cast<int*>(smem + LD::TB);
    float* sG = smem + LD::G;
    float* sEN0 = smem + LD::EN0;
    const Lane L = lane_info();
    const int tid = L.tid, n = L.n, g = L.g;
    const int b = blockIdx.x;
#ifdef GT_EXP_SAMESTATE   // timing experiment only (results are wrong): every workgroup works on the state of one of eight -- all
    float* stb = state + (long)(b & 7) * NS * ST_FLOATS;       // state traffic hits in L2: what the step costs without HBM latency
#else
    float* stb = state + (IDX ? 0L : (long)b * NS * ST_FLOATS);   // first stream of this workgroup (IDX: slot 0, see SROW)
#endif
    const int nlive = min(NS, NB - b * NS), nfr = nlive;
    [[maybe_unused]] volatile int* sSlot = reinterpret_cast<int*>(smem + LD::FLOATS);   // IDX: the slot ids (see SROW)
    if constexpr (IDX) {
        static_assert(NS <= SLOT_WORDS && (LD::FLOATS + SLOT_WORDS) * 4 <= 160 * 1024, "slot words behind the images");
        if (tid < SLOT_WORDS) sSlot[tid] = slots[b * NS + min(tid, nlive - 1)];
        wg_barrier();
    }
    const Tiles<TPW> tt = make_tiles<TPW, NWV>(L);
    int row[TPW], ffl[TPW];
    bool lane_live[TPW];
    [[maybe_unused]] float* stl[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        row[i] = min(tt.tl[i], NS - 1);                         // the lane's stream (lanes past the last stream: clamped)
        lane_live[i] = tt.tl[i] < nlive;
        stl[i] = stb + SROW(lane_live[i] ? tt.tl[i] : 0);
        ffl[i] = lane_live[i] ? tt.ff[i] : 0;
    }
#define STL(i) (IDX ? stb + SROW(lane_live[i] ? tt.tl[i] : 0) : stl[i])      // (as in k_stream_ms)

    constexpr int DN_PIECES = (SPLIT ? DN16_SIZE : 9 * 256) / 256;
    auto dense_fetch = [&](int j) {                                 // decoder block j's dense 3x3 -> stage buffer (see k_decoder)
        const float* src = PF + P_DEC + (SPLIT ? D_DN16 + j * DN16_SIZE : D_BLK + j * GBD_SIZE + GB_DN_A);
        int lz = L.lane;
        asm volatile("" : "+v"(lz));
        for (int pi = L.wave; pi < DN_PIECES; pi += NWV) lds_dma_1k(src + pi * 256 + 4 * lz, sDN + pi * 256);
    };
    // history rows of one block, all streams of the workgroup (k_stream_ms: hist_fetch / hist_store), HI items per thread
    constexpr int HI = (NS * 264 + NT - 1) / NT;
    auto hist_fetch = [&](int st_off, f32x4 (&v)[HI]) {
#pragma unroll
        for (int q = 0; q < HI; ++q) {
            const int i = tid + q * NT, sidx = i / 264, r = i - sidx * 264;
            const bool ok = i < NS * 264 && sidx < nlive;
            v[q] = ld4(stb + (ok ? SROW(sidx) + st_off + r * 4 : SROW(0) + ST_ENC_H));   // clamped: a valid record
        }
    };
    auto hist_store = [&](float* img, auto split, const f32x4 (&v)[HI]) {
        constexpr bool SP = decltype(split)::value;
        constexpr int RS = SP ? RS_WIDE : 16;
#pragma unroll
        for (int q = 0; q < HI; ++q) {
            const int i = tid + q * NT, sidx = i / 264, r = i - sidx * 264;
            if (i < NS * 264) {
                const int rw = r >= 132 ? 1 : 0, rr = r - rw * 132;
                const f32x4 val = sidx < nlive ? v[q] : splat(0.f);
                const int rec = (sidx * 2 * 35 + rw * 35 + 1 + (rr >> 2)) * RS;
                if constexpr (SP) st_split(img, rec, rr & 3, val);
                else st4(img + rec + 4 * (rr & 3), val);
            }
        }
    };
    auto hist_zero_pads = [&](float* img, int rs) {               // columns 0 and 34 of the NS * 2 image rows
        static_assert(NS * 2 * 2 * 8 <= NT, "one thread per 16-byte piece");
        if (tid < NS * 2 * 2 * 8) {
            const int rw = tid >> 4, side = (tid >> 3) & 1, gg = tid & 7;
            if (gg < rs / 4) st4(img + (rw * 35 + side * 34) * rs + 4 * gg, splat(0.f));
        }
    };
    // spectrogram items of a thread: element idx = tid + q * NT of the [stream][bin] step, bin fastest
    constexpr int SPEC_ITEMS = (NS * NBINS + NT - 1) / NT;
    auto spec_item = [&](int tz, int q, int& tq, int& f) {
        const int idx = tz + q * NT;
        tq = idx / NBINS;
        f = idx - tq * NBINS;
    };

    // ------------------------------------------------------------------------------------------------- prologue
    // group A  encoder front end (ERB bands, SFE, en_convs.0/1) -> P1, waited for at the first barrier
    // group B  the three encoder blocks -> P1, counted wait at the barrier behind en_conv1
    // group D0 the ERB.bs table and decoder block 0's dense planes -> their own buffers (first read in the decoder)
    // B and D0 are issued BEHIND the consumption of this phase's register loads (see lds_dma_1k)
    constexpr int DMA_A = ((E_BLK + 255) / 256 + NWV - 1) / NWV;
    constexpr int DMA_B = ((ENC_SIZE - E_BLK + 255) / 256 + NWV - 1) / NWV;
    constexpr int DMA_D0 = ((NBINS * 4 + 255) / 256 + DN_PIECES + NWV - 1) / NWV;   // (issued behind the GTCN, see there)
    {
        const DmaSeg ga[1] = {{P_ENC, LD::P1, E_BLK}};
        lds_dma_group<1, DMA_A, NWV>(ga, PF, smem, L.wave, L.lane);
    }
    for (int i = tid; i < P_INTS - ENC_I_SKIP; i += NT) sI[i] = PI[i < I_BS_LO ? i : i + ENC_I_SKIP];
    if (tid < NS * 48) {
        const int sidx = tid / 48, e = tid - sidx * 48;
        sEHe[tid] = sidx < nlive ? stb[SROW(sidx) + ST_ENC_E + e] : 0.f;
        sEHd[tid] = sidx < nlive ? stb[SROW(sidx) + ST_DEC_E + e] : 0.f;
    }
    if (tid < 8) sTB[tid] = tid < nlive ? reinterpret_cast<const int*>(stb + SROW(tid))[0] : 0;
    f32x4 hv[HI];
    hist_fetch(ST_ENC_H, hv);
    hist_zero_pads(smem + LD::HE, 16);

    // ------------------------------------------------------------------------------------------------- encoder
    float* sSpec = smem + LD::A;
    float* sE0 = smem + LD::A;
    float* sWe = smem + LD::A;
    float* sSe = smem + LD::SE;
    float* sEB = smem + LD::B;
    float* sF0 = sEB + 3 * RW * EB_ROW;
    const int sf32 = (int)sf, st32 = (int)sb;
    float2 spn[SPEC_ITEMS];                                        // kept for the mask at the end of the step
    {
        const float* base = spec + (long)b * NS * sb;
#pragma unroll
        for (int q = 0; q < SPEC_ITEMS; ++q) {
            int tl, f;
            spec_item(tid, q, tl, f);
            const bool ok = tl < nfr;                              // (f < NBINS by construction)
            spn[q] = *reinterpret_cast<const float2*>(base + (ok ? f * sf32 + tl * st32 : 0));
        }
    }
    hist_store(smem + LD::HE, std::false_type{}, hv);
    if (tid < 3 * RW * 9) {                                        // zero pad entries of EB / F0
        const int rw = tid / 9, e = tid - rw * 9;
        if (e < 2) sEB[rw * EB_ROW + e * 130] = 0.f;
        else sF0[rw * F0_ROW + (e < 4 ? e - 2 : 127 + e)] = 0.f;
    }
    {   // A0: [mag, re, im] of the new frames
#pragma unroll
        for (int q = 0; q < SPEC_ITEMS; ++q) {
            int tl, f;
            spec_item(tid, q, tl, f);
            if (tl < nfr) {
                const float2 v = spn[q];
                const bool low = f < ERB_LOW;
                float* d = low ? sEB + tl * EB_ROW + 1 + f : sSpec + tl * NBINS + f;
                const int cs = low ? RW * EB_ROW : RW * NBINS;
                d[0] = __builtin_amdgcn_sqrtf(v.x * v.x + v.y * v.y + 1e-12f);
                d[cs] = v.x;
                d[2 * cs] = v.y;
            }
        }
    }
    // the spectrogram items wait for the mask phase in LDS until the decoder starts (lane-private pieces in the dense stage
    // buffer and the ERB.bs table's place, both first needed by the decoder): eight registers less through the encoder
    // and the GTCN, the kernel's register peak
    float* sParkS = smem + LD::DN + 4 * tid;
    static_assert(SPEC_ITEMS % 2 == 0 && SPEC_ITEMS / 2 * NT * 4 <= LD::I - LD::DN, "parked spectrogram items fit DN + BS");
#pragma unroll
    for (int q = 0; q < SPEC_ITEMS; q += 2) {
        const f32x4 pk = {spn[q].x, spn[q].y, spn[q + 1].x, spn[q + 1].y};
        st4(sParkS + (q / 2) * NT * 4, pk);
    }
    {
        const DmaSeg gb[1] = {{P_ENC + E_BLK, LD::P1 + E_BLK, ENC_SIZE - E_BLK}};
        lds_dma_group<1, DMA_B, NWV>(gb, PF, smem, L.wave, L.lane);
    }
    wg_barrier_vm<DMA_B>();                                        // group A has landed; B stays in flight
    STAMP(SS, 0)
    {   // A: ERB.bm bands
        const int band = tid & (ERB_BANDS - 1);
        const int lo = sI[I_ERB_LO + band], cnt = sI[I_ERB_N + band];
        float w[ERB_MAXBW];
#pragma unroll
        for (int i = 0; i < ERB_MAXBW; i += 4) {
            const f32x4 t = ld4(sPE + E_ERB_W + band * ERB_MAXBW + i);
            w[i] = t[0]; w[i + 1] = t[1]; w[i + 2] = t[2]; w[i + 3] = t[3];
        }
        for (int ct = tid >> 6; ct < 3 * RW; ct += NWV) {
            if ((ct % RW) >= nfr) continue;
            const float* sp = sSpec + ct * NBINS + ERB_LOW + lo;
            float a0 = 0.f, a1 = 0.f;
#pragma unroll
            for (int i = 0; i < ERB_MAXBW; i += 2) {
                a0 += w[i] * (i < cnt ? sp[i] : 0.f);
                a1 += w[i + 1] * (i + 1 < cnt ? sp[i + 1] : 0.f);
            }
            sEB[ct * EB_ROW + 1 + ERB_LOW + band] = a0 + a1;
        }
    }
    wg_barrier();
    STAMP(SS, 1)
    // B: SFE_Lite
    for (int rw = L.wave; rw < 3 * RW; rw += NWV) {
        const int tl = rw % RW, c = rw / RW;
        if (tl >= nfr) continue;
        const float w0 = sPE[E_SFE_W + c * 3], w1 = sPE[E_SFE_W + c * 3 + 1], w2 = sPE[E_SFE_W + c * 3 + 2];
        const float* e = sEB + rw * EB_ROW;
        float* d = sF0 + rw * F0_ROW + 2;
        const int f = tid & 63;
        d[f] = w0 * e[f] + w1 * e[f + 1] + w2 * e[f + 2];
        d[f + 64] = w0 * e[f + 64] + w1 * e[f + 65] + w2 * e[f + 66];
        if (f == 0) d[128] = w0 * e[128] + w1 * e[129] + w2 * e[130];
    }
    if (tid < RW * 4 * 4) {                                        // pad positions of E0
        const int r = tid >> 4, cc = (tid >> 2) & 3, gg = tid & 3;
        st4(sE0 + pl(r * ENC_E0_ROW + (cc < 2 ? cc : 65 + cc), gg), splat(0.f));
    }
    wg_barrier();
    STAMP(SS, 2)
    {   // C: en_convs.0; en0 stays in LDS for the decoder tail
        const f32x4 A = ld4(sPE + E_EN0_A + arow(n, g)), Bv = ld4(sPE + E_EN0_B + 4 * g);
        const float a = sPE[E_EN0_S] - 1.0f;
        int off[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int e = 4 * g + s, c = e < 15 ? e / 5 : 0, k = e < 15 ? e % 5 : 0;
            off[s] = c * RW * F0_ROW + k;
        }
        const int nt0 = (nfr * F1 + 15) >> 4;
        for (int tile = L.wave; tile < nt0; tile += NWV) {
            const int q = tile * 16 + n;
            int tl = q / F1;
            const int fo = q - tl * F1;
            if (tl >= RW) tl = RW - 1;
            f32x4 bv;
#pragma unroll
            for (int s = 0; s < 4; ++s) bv[s] = sF0[off[s] + tl * F0_ROW + 2 * fo];
            f32x4 acc = mm1<false>(A, bv, Bv);
            acc = prelu4(acc, a);
            if (q < RW * F1) st4(sE0 + pl(tl * ENC_E0_ROW + 2 + fo, g), acc);
            if (q < nfr * F1) st4(sEN0 + q * 16 + 4 * g, acc);
        }
    }
    wg_barrier();
    STAMP(SS, 3)
    f32x4 x[TPW], en1p[TPW], en2p[TPW], en3p[TPW];
    {   // D: en_convs.1; en1 is kept in the slot order of its decoder consumer
        const f32x4 Bv = ld4(sPE + E_EN1_B + 4 * g);
        const float a = sPE[E_EN1_S] - 1.0f;
        const int* ix = sI + I_ENST - ENC_I_SKIP + 0 * 16 + 4 * g;
#pragma unroll
        for (int i = 0; i < TPW; ++i) x[i] = Bv;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const f32x4 A = ld4(sPE + E_EN1_A + k * 256 + arow(n, g));
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                const f32x4 tap = ld4(sE0 + pl(row[i] * ENC_E0_ROW + 2 * tt.ff[i], g) + k * 16);
                x[i] = mm1<false>(A, tap, x[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            x[i] = prelu4(x[i], a);
            en1p[i] = permute_via_lds(sEB + (L.wave * 16 + n) * PERM_RS, ix, g, x[i]);
        }
    }
    wg_barrier_vm<0>();                                            // E0, EB, F0 are dead; group B (block parameters) has landed
    STAMP(SS, 4)
    // group C: both GTCN stacks -> the EB / F0 region; first read behind the last encoder block's closing barrier
    {
        constexpr int DMA_C = ((2 * GTCN_SIZE + 255) / 256 + NWV - 1) / NWV;
        const DmaSeg gc[1] = {{P_GTCN, LD::GP, 2 * GTCN_SIZE}};
        lds_dma_group<1, DMA_C, NWV>(gc, PF, smem, L.wave, L.lane);
    }
    zero_row_pads<RW, 16, 35>(sWe, tid);
    // GTCN history rows of the lane's positions (k_gtcn_ms): requested during the last encoder block
    int tbl[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) tbl[i] = sTB[row[i]];
    f32x4 t1[4][TPW], t2[4][TPW];
    int r2[4][TPW];
    // (all sixteen loads per thread at the top of the last encoder block; spreading them over the block's phases or over
    // two blocks was tried: the longer live ranges push 19 .. 45 registers into scratch; block 0's rows at the top and the
    // other twelve behind the block's second barrier compiles without scratch and is +-0 at 16 384 streams, -1.5 % at
    // 65 536, +0.5 % at 1 792: not kept)
    auto fetch_rows = [&](int st_off, auto kc) {
        constexpr int k = decltype(kc)::value;
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const float* ring = STL(i) + st_off;
            constexpr int d = 1 << k, m2d = 2 * d - 1, row0 = 2 * (d - 1);
            const int r1 = ((row0 + ((tbl[i] + d) & m2d)) * 33 + ffl[i]) * 16 + 4 * g;
            r2[k][i] = ((row0 + (tbl[i] & m2d)) * 33 + ffl[i]) * 16 + 4 * g;
            t1[k][i] = ld4(ring + r1);
            t2[k][i] = ld4(ring + r2[k][i]);
        }
    };
    auto fill_ctx = [&](BlockCtx& c, const float* pb, const float* gA, const int* ib, float* sW, float* sS, float* sEHk,
                        int roff0, int hrs, int st_h, int blk) {
        c.pb = pb; c.gA = gA; c.ib = ib;
        c.sW = sW; c.sHk = nullptr; c.sS = sS; c.sG = sG; c.sEHk = sEHk;
        c.sHtop = nullptr; c.sHnext = nullptr;
        c.sE = smem + LD::E;
        c.sY = sG + CF::RWG * 16;
        c.nfr = nfr; c.tabs = 0;
        c.sTB = sTB;
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            c.ms_roff[i] = roff0 + row[i] * (2 * 35 * hrs);
            c.ms_tb[i] = tbl[i];
            c.g_hist[i] = STL(i) + st_h + ((blk * 2 + (tbl[i] & 1)) * 33 + ffl[i]) * 16 + 4 * g;
        }
    };
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        BlockCtx c;
        fill_ctx(c, sPE + E_BLK + k * GB_SIZE, nullptr, sI + I_ENC_BLK - ENC_I_SKIP + k * 16, sWe, sSe, sEHe + k * 16,
                 (int)(smem + LD::HE - sWe), 16, ST_ENC_H, k);
        if (k < 2) hist_fetch(ST_ENC_H + (k + 1) * 2 * 33 * 16, hv);
        if (k == 2) {
            fetch_rows(ST_G1_H, std::integral_constant<int, 0>{});
            fetch_rows(ST_G1_H, std::integral_constant<int, 1>{});
            fetch_rows(ST_G1_H, std::integral_constant<int, 2>{});
            fetch_rows(ST_G1_H, std::integral_constant<int, 3>{});
        }
        // (k == 2: the closing barrier also waits for the wave's vector memory: the GTCN parameters -- issued two blocks
        // ago -- are then visible to every wave; the row loads above are a block old by then)
        if (k < 2)
            gtconv_block<false, TPW, true, false, 16, 16, true, 35, 0, -1, NWV, PMAX, -1>(
                x, tt, c, L, [] {}, [&] { hist_store(smem + LD::HE, std::false_type{}, hv); } STAMP_ARG);
        else
            gtconv_block<false, TPW, true, false, 16, 16, true, 35, 0, -1, NWV, PMAX, 0>(
                x, tt, c, L, [] {}, [] {} STAMP_ARG);
        if (k < 2) {
            const int* ix = sI + I_ENST - ENC_I_SKIP + (k + 1) * 16 + 4 * g;
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                // (wave-private scratch inside S: free from the block's closing barrier to the next block's second phase)
                const f32x4 y = permute_via_lds(sSe + (L.wave * 16 + n) * PERM_RS, ix, g, x[i]);
                if (k == 0) en2p[i] = y; else en3p[i] = y;
            }
        }
        STAMP(SS, 8)
    }
#ifdef GT_STAMPS
    SS.acc[10] = SS.acc[5]; SS.acc[11] = SS.acc[6]; SS.acc[12] = SS.acc[7];
    SS.acc[5] = SS.acc[6] = SS.acc[7] = 0;
#endif
    // ------------------------------------------------------------------------------------------------- GTCN x 2
    // every wave is behind the encoder's last barrier: the encoder parameters are dead, P1 takes the decoder's blocks
    // (without their dense matrices) and the de_convs.3/4 segment -- group D1, first read behind the barrier after the GTCN
    {
        constexpr int D1_PIECES = 3 * ((GB_SIZE + 255) / 256) + (SPLIT3 ? DE3_16_MATS : 5) + (D_BS_W - D_DE3_B + 255) / 256;
        constexpr int DMA_D1 = (D1_PIECES + NWV - 1) / NWV;
        const DmaSeg gd[5] = {{P_DEC + D_BLK + 0 * GBD_SIZE, LD::P1 + 0 * GB_SIZE, GB_SIZE},
                              {P_DEC + D_BLK + 1 * GBD_SIZE, LD::P1 + 1 * GB_SIZE, GB_SIZE},
                              {P_DEC + D_BLK + 2 * GBD_SIZE, LD::P1 + 2 * GB_SIZE, GB_SIZE},
                              {P_DEC + (SPLIT3 ? D_DE3_16 : D_DE3_AE), LD::P1 + DL_DE3M, SPLIT3 ? DE3_16_MATS * 256 : 5 * 256},
                              {P_DEC + D_DE3_B, LD::P1 + DL_DE, D_BS_W - D_DE3_B}};
        lds_dma_group<5, DMA_D1, NWV>(gd, PF, smem, L.wave, L.lane);
    }
    // The three skips wait out the GTCN in LDS (lane-private 16-byte pieces in the dead encoder images, no barrier: a lane
    // reads back what it wrote): with the rows of four TCN blocks x two tiles in registers the GTCN is the kernel's
    // register peak, and the skips -- live from the encoder to the decoder -- would otherwise go to scratch.
    float* sPark = smem + LD::X + 4 * tid;
    static_assert(3 * TPW * NT * 4 <= LD::GP - LD::X, "parked skips fit the dead encoder images");
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        st4(sPark + (0 * TPW + i) * NT * 4, en1p[i]);
        st4(sPark + (1 * TPW + i) * NT * 4, en2p[i]);
        st4(sPark + (2 * TPW + i) * NT * 4, en3p[i]);
    }
    {
        f32x4 x0[TPW];
#pragma unroll
        for (int i = 0; i < TPW; ++i) x0[i] = x[i];
#pragma unroll
        for (int stack = 0; stack < 2; ++stack) {
            const int st_off = stack == 0 ? ST_G1_H : ST_G2_H;
            const float* pk = sPG + stack * GTCN_SIZE;
            // (the second stack's rows of block k are requested as soon as the first stack's block k has used its own: the
            // same registers, four blocks of lead time -- holding both stacks' rows at once does not fit 256 VGPRs)
            auto blk = [&](auto kc, auto dc) {
                constexpr int k = decltype(kc)::value, D = decltype(dc)::value;
                float* q2[TPW];
#pragma unroll
                for (int i = 0; i < TPW; ++i) q2[i] = STL(i) + st_off + r2[k][i];
                tcn_block_msn<D, TPW>(x, pk + k * TCN_SIZE, t1[k], t2[k], q2, lane_live, n, g);
                // (one TCN block's parameter reads in flight at a time: hoisted across blocks they push the long-lived skips
                // and the spectrogram into scratch)
                __builtin_amdgcn_sched_barrier(0);
                if (stack == 0) {
#pragma unroll
                    for (int i = 0; i < TPW; ++i) {
                        const float* ring = STL(i) + ST_G2_H;
                        constexpr int m2d = 2 * D - 1, row0 = 2 * (D - 1);
                        t1[k][i] = ld4(ring + ((row0 + ((tbl[i] + D) & m2d)) * 33 + ffl[i]) * 16 + 4 * g);
                        t2[k][i] = ld4(ring + r2[k][i]);
                    }
                }
            };
#ifdef GT_STAMPS_GTCN      // (diagnostic: the eight TCN blocks of the step in stamp slots 0 .. 7 instead of the phase sums)
#define GTCN_STAMP(i) if (stack == 0) STAMP(SS, i) else STAMP(SS, 4 + i)
            if (stack == 0) {
#pragma unroll
                for (int k_ = 0; k_ < 16; ++k_) SS.acc[k_] = 0;
                SS.t = __builtin_amdgcn_s_memtime();
            }
#else
#define GTCN_STAMP(i)
#endif
            blk(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
            GTCN_STAMP(0)
            blk(std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{});
            GTCN_STAMP(1)
            // the decoder's first history image: requested where the second stack has released half of its row registers
            if (stack == 1) hist_fetch(ST_DEC_H, hv);
            blk(std::integral_constant<int, 2>{}, std::integral_constant<int, 4>{});
            GTCN_STAMP(2)
            blk(std::integral_constant<int, 3>{}, std::integral_constant<int, 8>{});
            GTCN_STAMP(3)
#undef GTCN_STAMP
        }
#pragma unroll
        for (int i = 0; i < TPW; ++i) x[i] = x[i] + x0[i];         // gtcn2(gtcn1(x)) + en_outs[4] (Decoder.forward :467)
    }
#pragma unroll
    for (int i = 0; i < TPW; ++i) {                                // the skips come back before the decoder's images take the region
        en1p[i] = ld4(sPark + (0 * TPW + i) * NT * 4);
        en2p[i] = ld4(sPark + (1 * TPW + i) * NT * 4);
        en3p[i] = ld4(sPark + (2 * TPW + i) * NT * 4);
    }
#pragma unroll
    for (int q = 0; q < SPEC_ITEMS; q += 2) {
        const f32x4 pk = ld4(sParkS + (q / 2) * NT * 4);
        spn[q] = make_float2(pk[0], pk[1]);
        spn[q + 1] = make_float2(pk[2], pk[3]);
    }
    __builtin_amdgcn_sched_barrier(0);
#ifdef GT_STAMPS_GTCN
    STAMP_OUT(SS, stamps)
    stamps = nullptr;
#endif
    STAMP(SS, 9)
    // ------------------------------------------------------------------------------------------------- decoder
    constexpr int RS = LD::RSD;
    float* sHd = smem + LD::HD;
    float* sW = smem + LD::W;
    float* sS = smem + LD::SD;
    float* sZ = smem + LD::W;
    float* sM = smem + LD::M;
    constexpr int ZS = DEC_ZS;
    // Behind this barrier every wave has left the GTCN: its parameters and the parked skips are dead, the region takes the
    // decoder's images (block 0 reads them behind its first barrier); group D1 has landed: every wave has issued twenty
    // loads behind it (the second stack's rows, the history image), so "at most four outstanding" retires it and leaves
    // only the last two TCN blocks' ring stores in flight.
    wg_barrier_vm<2 * TPW>();
    {   // group D0: the ERB.bs table and block 0's dense planes take the place of the parked spectrogram items; every wave
        // issues the HI history loads of block 1 behind it, so block 0's first barrier (VMK1 = HI) retires it
        const DmaSeg gd[2] = {{P_DEC + D_BS_TAB, LD::BS, NBINS * 4},
                              {P_DEC + (SPLIT ? D_DN16 : D_BLK + GB_DN_A), LD::DN, DN_PIECES * 256}};
        lds_dma_group<2, DMA_D0, NWV>(gd, PF, smem, L.wave, L.lane);
    }
    hist_zero_pads(sHd, RS);
    if constexpr (SPLIT) hist_store(sHd, std::true_type{}, hv);
    else hist_store(sHd, std::false_type{}, hv);
    zero_row_pads<RW, RS>(sW, tid);
    STAMP(SS, 13)
    const int npos = nfr * 33;
    f32x4 s0e[TPW], s0o[TPW];
    auto run_block = [&](int j, const f32x4 (&skv)[TPW], auto&& hook, auto&& hook3, auto vmk1) {
        BlockCtx c;
        fill_ctx(c, sPD + j * GB_SIZE, sDN, sI + I_DEC_BLK - ENC_I_SKIP + j * 16, sW, sS, sEHd + j * 16, (int)(sHd - sW), RS,
                 ST_DEC_H, j);
        gtconv_block<true, TPW, true, false, RS, 16, true, 35, 0, decltype(vmk1)::value, NWV, PMAX>(
            x, tt, c, L, [&] { if (j < 2) dense_fetch(j + 1); hook(); }, hook3 STAMP_ARG);
#pragma unroll
        for (int i = 0; i < TPW; ++i) x[i] = x[i] + skv[i];
        STAMP(SS, 8)
    };
    // (first-barrier wait of a block = the vector-memory operations EVERY wave issues behind the DMA of its planes: blocks
    // 0 and 1 the HI history loads of the next block; block 2 none)
    hist_fetch(ST_DEC_H + 1 * 2 * 33 * 16, hv);
    run_block(0, en3p, [] {},
              [&] { if constexpr (SPLIT) hist_store(sHd, std::true_type{}, hv); else hist_store(sHd, std::false_type{}, hv); },
              std::integral_constant<int, HI>{});
    hist_fetch(ST_DEC_H + 2 * 2 * 33 * 16, hv);
    run_block(1, en2p, [] {},
              [&] { if constexpr (SPLIT) hist_store(sHd, std::true_type{}, hv); else hist_store(sHd, std::false_type{}, hv); },
              std::integral_constant<int, HI>{});
    run_block(2, en1p, [&] {
        // en_outs[0] for the even / odd output bins of the lane's positions, from LDS
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int o0 = (tt.pp(i) < npos ? tt.tl[i] * F1 + 2 * tt.ff[i] : 0) * 16 + 4 * g;
            s0e[i] = ld4(sEN0 + o0);
            s0o[i] = ld4(sEN0 + o0 + (tt.ff[i] < 32 ? 16 : 0));
        }
    }, [] {}, std::integral_constant<int, 0>{});
    // ---- de_convs.3 (gather form) + de_convs.4 (scatter form)
    int rec3[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        rec3[i] = o35<RS, 0>(tt, i, 0);
        if (i < TPW - 1 || tt.pp(i) < PMAX) {
            if constexpr (SPLIT3) st_split(sW, rec3[i], g, x[i]);
            else st4(sW + rec3[i] + 4 * g, x[i]);
        }
    }
    wg_barrier();
    f32x4 ze[TPW], zo[TPW];
    {
        const f32x4 Bv = ld4(sPD + dl(D_DE3_B) + 4 * g);
        const float a = sPD[dl(D_DE3_S)] - 1.0f;
        f32x4 ae[TPW], ao[TPW];
        de_conv3_tiles<TPW, SPLIT3, false, RS>(sW, rec3, x, sPD + DL_DE3M, Bv, n, g, ae, ao);
        const f32x4 A4 = ld4(sPD + dl(D_DE4_A) + arow(n, g));
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            f32x4 e2 = prelu4(ae[i], a), o2 = prelu4(ao[i], a);
            e2 = e2 + s0e[i];
            o2 = o2 + s0o[i];
            ze[i] = mm1<false>(A4, e2, splat(0.f));
            zo[i] = mm1<false>(A4, o2, splat(0.f));
        }
    }
    wg_barrier();                                                  // region W becomes Z
    if (g < 3) {
#pragma unroll
        for (int i = 0; i < TPW; ++i)
            if (i < TPW - 1 || tt.pp(i) < PMAX) {
                st4(sZ + (tt.tl[i] * DEC_Z_ROW + 1 + 2 * tt.ff[i]) * ZS + 4 * g, ze[i]);
                if (tt.ff[i] < 32) st4(sZ + (tt.tl[i] * DEC_Z_ROW + 2 + 2 * tt.ff[i]) * ZS + 4 * g, zo[i]);
            }
    }
    if (tid < RW * 2 * 4 && (tid & 3) < 3)
        st4(sZ + ((tid >> 3) * DEC_Z_ROW + ((tid >> 2) & 1) * (DEC_Z_ROW - 1)) * ZS + 4 * (tid & 3), splat(0.f));
    wg_barrier();
    {   // de_convs.4 gather + BN + Tanh: item = (stream row, output channel o, bin f'')
        for (int idx = tid; idx < RW * 2 * F0; idx += NT) {
            const int h = idx / (2 * F0), c = idx - h * (2 * F0), o = c >= F0 ? 1 : 0, fq = c - o * F0;
            const int par = fq & 1, m = fq >> 1;
            const float* zr = sZ + (h * DEC_Z_ROW + 1 + m) * ZS;
            const float* r1 = zr + ZS + o * 5 + par;
            const float* r2p = zr + o * 5 + 2 + par;
            const float* r3 = zr - ZS + (par ? 10 : o * 5 + 4);
            const float bias = sPD[dl(D_DE4_B) + o];
            const float sum = bias + r1[0] + r2p[0] + r3[0];
            sM[(o * RW + h) * F0 + fq] = fast_tanh(sum);
        }
    }
    wg_barrier();
    STAMP(SS, 14)
    {   // ERB.bs + complex ratio mask + output layout
        float* obase = out + (long)b * NS * osb;
        const int osf32 = (int)osf, ost32 = (int)osb;
        int tz = tid;                                              // (opaque: the items' (stream, bin) are recomputed here,
        asm volatile("" : "+v"(tz));                               //  not kept live -- in scratch -- since the prologue)
#pragma unroll
        for (int q = 0; q < SPEC_ITEMS; ++q) {
            int tq, f;
            spec_item(tz, q, tq, f);
            const bool ok = tq < nfr;
            const int tc = ok ? tq : 0;
            const f32x4 tb = ld4(sBS + f * 4);
            const float* mp = sM + tc * F0 + __float_as_int(tb[0]);
            const float a0 = mp[0], a1 = mp[1], b0 = mp[RW * F0], b1 = mp[RW * F0 + 1];
            const bool two = tb[2] != 0.f;
            const float mr = tb[1] * a0 + (two ? tb[2] * a1 : 0.f);
            const float mi = tb[1] * b0 + (two ? tb[2] * b1 : 0.f);
            const float re = spn[q].x, im = spn[q].y;
            const float yr = re * mr - im * mi, yi = im * mr + re * mi;
            if (ok) *reinterpret_cast<float2*>(obase + f * osf32 + tq * ost32) = make_float2(yr, yi);
        }
    }
    // ------------------------------------------------------------------------------------------------- epilogue
    if (tid < nlive * 48) {
        const int sidx = tid / 48, e = tid - sidx * 48;
        stb[SROW(sidx) + ST_ENC_E + e] = sEHe[tid];
        stb[SROW(sidx) + ST_DEC_E + e] = sEHd[tid];
    }
    if (tid < nlive) reinterpret_cast<int*>(stb + SROW(tid))[0] = (sTB[tid] + 1) & 0xFFFF;
    STAMP(SS, 15)
    STAMP_OUT(SS, stamps)
}

#undef STL
#undef SROW
// ==================================================================== stream slots: reset
// Zeroes the model state and (wstate != nullptr) the wave state of the listed slots: what gtcrn_stream_reset does to a
// contiguous range with a memset, as a kernel, so that a captured graph admits a stream at any slot.  RESET_PARTS workgroups
// share one slot's 152 KB (blockIdx.y), 16-byte stores; rows at or beyond the clamped count are left alone.
constexpr int RESET_PARTS = 8;
static_assert(ST_FLOATS % 4 == 0 && WS_FLOATS % 4 == 0, "whole 16-byte pieces");
__global__ __launch_bounds__(256) void k_reset_slots(float* __restrict__ state, float* __restrict__ wstate,
                                                     const int* __restrict__ slots, const int* __restrict__ cnt,
                                                     int max_active) {
    const int n = blockIdx.x, part = blockIdx.y, tid = threadIdx.x;
    if (n >= slot_count(cnt, max_active)) return;
    const long slot = slots[n];
    constexpr int PIECES = ST_FLOATS / 4, PER = (PIECES + RESET_PARTS - 1) / RESET_PARTS;
    f32x4* st = reinterpret_cast<f32x4*>(state + slot * ST_FLOATS);
    const int hi = min(PIECES, (part + 1) * PER);
    for (int i = part * PER + tid; i < hi; i += 256) st[i] = splat(0.f);
    if (wstate && part == RESET_PARTS - 1) {                      // (the last part holds the short share of the model state)
        f32x4* ws = reinterpret_cast<f32x4*>(wstate + slot * WS_FLOATS);
        for (int i = tid; i < WS_FLOATS / 4; i += 256) ws[i] = splat(0.f);
    }
}

// ==================================================================== state conversion
// library ring state <-> the reference's caches (gtcrn_micro_stream.py:618-623, slices :416-428
// and :490-500).  dir 0: import (reference -> rings), 1: export.  One workgroup per stream.
__global__ void k_state_convert(float* __restrict__ state, int N, float* __restrict__ conv, float* __restrict__ tra,
                                float* const* __restrict__ tcn8, const int* __restrict__ PI, int dir) {
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    float* st = state + (long)b * ST_FLOATS;
    int pos = dir == 0 ? 0 : reinterpret_cast<const int*>(st)[0];
    if (dir == 0 && tid == 0) reinterpret_cast<int*>(st)[0] = 0;
    // conv_cache (2,N,16,6,33): encoder block k rows 2k..2k+1, decoder block j rows 4-2j..5-2j;
    // the cached tensor is h (hidden channel order == slot order); cache row r holds frame pos-2+r.
    for (int e = 0; e < 2; ++e)
        for (int idx = tid; idx < 3 * 2 * 33 * 16; idx += nthr) {
            const int s = idx & 15, f = (idx >> 4) % 33, r = ((idx >> 4) / 33) & 1, k = (idx >> 4) / 66;
            const int row = (e == 0 ? 2 * k : 4 - 2 * k) + r;
            float* c = conv + ((((long)e * N + b) * 16 + s) * 6 + row) * 33 + f;
            float* rg = st + (e == 0 ? ST_ENC_H : ST_DEC_H) + ((k * 2 + ((pos - 2 + r) & 1)) * 33 + f) * 16 + s;
            if (dir == 0) *rg = *c; else *c = *rg;
        }
    // tra_cache (2,3,N,8,2): last two energies, entry r holds frame pos-2+r
    for (int idx = tid; idx < 2 * 3 * 8 * 2; idx += nthr) {
        const int r = idx & 1, c8 = (idx >> 1) & 7, k = (idx >> 4) % 3, e = idx / 48;
        float* c = tra + ((((long)e * 3 + k) * N + b) * 8 + c8) * 2 + r;
        float* rg = st + (e == 0 ? ST_ENC_E : ST_DEC_E) + k * 16 + ((pos - 2 + r) & 1) * 8 + c8;
        if (dir == 0) *rg = *c; else *c = *rg;
    }
    // tcn_cache[g][k] (N,16,2d,33): y1 (hidden order), row r holds frame pos-2d+r
    for (int gk = 0; gk < 8; ++gk) {
        const int gg = gk >> 2, k = gk & 3, d = 1 << k;
        float* cache = tcn8[gk];
        for (int idx = tid; idx < 2 * d * 33 * 16; idx += nthr) {
            const int s = idx & 15, f = (idx >> 4) % 33, r = (idx >> 4) / 33;
            float* c = cache + (((long)b * 16 + s) * 2 * d + r) * 33 + f;
            float* rg = st + (gg == 0 ? ST_G1_H : ST_G2_H) + ((2 * (d - 1) + ((pos - 2 * d + r) & (2 * d - 1))) * 33 + f) * 16 + s;
            if (dir == 0) *rg = *c; else *c = *rg;
        }
    }
    (void)PI;
}

// ===================================================================== generic causal conv (wrappers)
// StreamConv2d.forward / StreamConvTranspose2d.forward (streaming/conversion/convolution.py:107-119,
// 201-253) for arbitrary small shapes: input = cat([cache, x]) along time, VALID convolution in time,
// zero padding pf in frequency, stride 1, dilation (dt, df), groups; the new cache is the last
// (kt-1)*dt rows of the input.  transposed = 1 computes ConvTranspose2d semantics directly from the
// (in, out, kt, kf) weight: y[o,t,f] = b[o] + sum x[i, t - a*dt, f + pf - q*df] W[i,o,a,q], which is
// what the reference obtains from Conv2d with permuted + flipped weights (convert.py:35-48).
// One thread per output element; these wrappers are not on the fused hot path.
__global__ void k_conv2d_causal(const float* __restrict__ x, const float* __restrict__ cache,
                                const float* __restrict__ w, const float* __restrict__ bias,
                                float* __restrict__ y, float* __restrict__ cache_out, int B, int Cin, int Cout, int T,
                                int F, int kt, int kf, int dt, int df, int pf, int groups, int transposed, int Fout) {
    const int H = (kt - 1) * dt;
    const long total = (long)B * Cout * T * Fout;
    const int cpg = Cin / groups, opg = Cout / groups;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int f = (int)(idx % Fout);
        const int t = (int)((idx / Fout) % T);
        const int o = (int)((idx / ((long)Fout * T)) % Cout);
        const int b = (int)(idx / ((long)Fout * T * Cout));
        float acc = bias ? bias[o] : 0.f;
        const int gq = transposed ? 0 : o / opg;
        const int ci0 = transposed ? 0 : gq * cpg, nci = transposed ? Cin : cpg;
        for (int ci = 0; ci < nci; ++ci) {
            const int c = ci0 + ci;
            for (int a = 0; a < kt; ++a) {
                const int tau = transposed ? t - a * dt : t - H + a * dt;   // frame relative to the chunk start
                const float* row = tau >= 0 ? x + (((long)b * Cin + c) * T + tau) * F
                                            : cache + (((long)b * Cin + c) * H + (H + tau)) * F;
                for (int q = 0; q < kf; ++q) {
                    const int fi = transposed ? f + pf - q * df : f - pf + q * df;
                    if (fi >= 0 && fi < F) {
                        const float wv = transposed ? w[(((long)c * Cout + o) * kt + a) * kf + q]
                                                    : w[(((long)o * cpg + ci) * kt + a) * kf + q];
                        acc += wv * row[fi];
                    }
                }
            }
        }
        y[idx] = acc;
    }
    // new cache = last H rows of [cache | x]
    const long ctotal = (long)B * Cin * H * F;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < ctotal; idx += (long)gridDim.x * blockDim.x) {
        const int f = (int)(idx % F);
        const int r = (int)((idx / F) % H);
        const long bc = idx / ((long)F * H);
        const int tau = T - H + r;
        cache_out[idx] = tau >= 0 ? x[(bc * T + tau) * F + f] : cache[(bc * H + (H + tau)) * F + f];
    }
}

// ==================================================================================== self test
// D = A(16x4) * B(4x16) + C with the lane maps the kernels rely on:
// a = A[i = lane&15][k = lane>>4], b = B[k = lane>>4][j = lane&15], D reg r -> row 4*(lane>>4)+r, col lane&15.
__global__ void k_selftest(const float* __restrict__ A, const float* __restrict__ Bm, const float* __restrict__ C,
                           float* __restrict__ D) {
    const int lane = threadIdx.x, n = lane & 15, g = lane >> 4;
    f32x4 c;
#pragma unroll
    for (int r = 0; r < 4; ++r) c[r] = C[(4 * g + r) * 16 + n];
    c = mfma(A[n * 4 + g], Bm[g * 16 + n], c);
#pragma unroll
    for (int r = 0; r < 4; ++r) D[(4 * g + r) * 16 + n] = c[r];
}

// split3 / join3 / split_mm6 on caller-chosen values (gtcrn_selftest_split3): element i -> its three bf16 planes (as
// floats) and the re-joined value; and D (16x16) = A (16x32) * B (32x16) through the six-product helper from operands
// split ON THE DEVICE, with the lane maps of the dense 3x3 (A fragment: row n, k = 8g..8g+7; B: column n, k = 8g..8g+7).
__global__ void k_selftest_split3(const float* __restrict__ x, long n, float* __restrict__ planes,
                                  float* __restrict__ joined, const float* __restrict__ A,
                                  const float* __restrict__ Bm, float* __restrict__ D) {
    for (long i = 4L * (blockIdx.x * blockDim.x + threadIdx.x); i < n; i += 4L * gridDim.x * blockDim.x) {
        const f32x4 v = ld4(x + i);
        const Split3 s = split3(v);
        const f32x4 j = join3(s.h, s.m, s.l);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            planes[i + e] = (float)s.h[e];
            planes[n + i + e] = (float)s.m[e];
            planes[2 * n + i + e] = (float)s.l[e];
        }
        st4(joined + i, j);
    }
    if (blockIdx.x == 0 && threadIdx.x < 64 && A) {
        const int lane = threadIdx.x, nn = lane & 15, g = lane >> 4;
        bf16x8 ap[3], bp[3];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const Split3 sa = split3(ld4(A + nn * 32 + 8 * g + 4 * h));
            f32x4 bv;
#pragma unroll
            for (int e = 0; e < 4; ++e) bv[e] = Bm[(8 * g + 4 * h + e) * 16 + nn];
            const Split3 sb = split3(bv);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ap[0][4 * h + e] = sa.h[e]; ap[1][4 * h + e] = sa.m[e]; ap[2][4 * h + e] = sa.l[e];
                bp[0][4 * h + e] = sb.h[e]; bp[1][4 * h + e] = sb.m[e]; bp[2][4 * h + e] = sb.l[e];
            }
        }
        const f32x4 c = split_mm6(ap, bp, splat(0.f));
#pragma unroll
        for (int r = 0; r < 4; ++r) D[(4 * g + r) * 16 + nn] = c[r];
    }
}

// Prefix table of a variable-length batch for the time spans (span_begin): pref[b] = frames of utterances [0, b), with
// utterance b holding min(T, 1 + (lens[b] >> 8)) frames (lens in samples, the STFT's frame count).  One workgroup,
// B <= PREF_MAX_B.
constexpr int PREF_MAX_B = 1024;
__global__ __launch_bounds__(PREF_MAX_B) void k_len_prefix(const int* __restrict__ lens, int B, int T, int* __restrict__ pref) {
    __shared__ int sc[PREF_MAX_B];
    const int i = threadIdx.x;
    int v = 0;
    if (i < B) {
        const int l = lens[i];
        v = l < 0 ? 0 : min(T, 1 + (l >> 8));
    }
    sc[i] = v;
    __syncthreads();
    for (int d = 1; d < PREF_MAX_B; d <<= 1) {          // inclusive scan, ten doubling steps
        const int add = i >= d ? sc[i - d] : 0;
        __syncthreads();
        sc[i] += add;
        __syncthreads();
    }
    if (i < B) pref[i + 1] = sc[i];
    if (i == 0) pref[0] = 0;
}

}  // namespace gtk

// ============================================================================== launchers
namespace gtk {

#define GT_LAUNCH_CHECK()                       \
    do {                                        \
        hipError_t e_ = hipGetLastError();      \
        if (e_ != hipSuccess) return (int)e_;   \
    } while (0)

// How an offline launch of a per-utterance kernel covers B utterances of T frames (see span_begin):
//   nA    utterances [0, nA) run one workgroup per utterance (no warm-up) -- whole rounds of 256, or everything;
//   nwgB  workgroups share the (utterance, frame) axis of the remaining B - nA utterances (0: none remain).
// Candidates: everything one per utterance; everything in 256 k shares; the whole rounds one per utterance and only the
// remainder in shares (B = 257: 256 + 1 -- a second launch of the same kernel on offset pointers).  Modelled time: rounds
// of 256 workgroups x 16-frame chunks walked (share + warm-up, one more chunk when shares cross utterance boundaries).
struct SpanPlan {
    int nA, nwgB;
};
static long span_chunks(long frames) { return (frames + TC - 1) / TC * TC; }
// (every round of workgroups also pays its prologue once -- parameters into LDS, rings zeroed, the first loads' latency:
// about half a chunk; without the term a plan of several rounds of one-frame shares looked as cheap as one round)
constexpr long SPAN_ROUND_FIXED = TC / 2;
static long spans_cost(int nu, int T, int halo, int nwg) {
    const long total = (long)nu * T, per = (total + nwg - 1) / nwg;
    return (long)(nwg / 256) * (span_chunks(per + halo) + ((T % per) ? TC : 0) + SPAN_ROUND_FIXED);
}
static int best_spans(int nu, int T, int halo, long* cost) {
    int best = 0;
    *cost = 0;
    for (int k = 1; k <= 8; ++k) {
        const int nwg = 256 * k;
        if (nwg < nu) continue;
        const long per = ((long)nu * T + nwg - 1) / nwg;
        if (per < 4 && best) break;                            // (shares of a few frames: all warm-up)
        const long c = spans_cost(nu, T, halo, nwg);
        if (!best || c < *cost) { *cost = c; best = nwg; }
    }
    return best;
}
static SpanPlan span_plan(int B, int T, int halo, bool allowed) {
    SpanPlan p{B, 0};
    if (!allowed) return p;
    long best = (long)((B + 255) / 256) * (span_chunks(T) + SPAN_ROUND_FIXED), c = 0;
    const int all = best_spans(B, T, halo, &c);
    if (all && c < best) { best = c; p = SpanPlan{0, all}; }
    const int q = B / 256, r = B % 256;
    if (q >= 1 && r > 0) {
        const int rem = best_spans(r, T, halo, &c);
        if (rem && (long)q * (span_chunks(T) + SPAN_ROUND_FIXED) + c < best) p = SpanPlan{256 * q, rem};
    }
    return p;
}
int span_workgroups(int B, int T, int halo, bool allowed) {      // (diagnostics: the share count of a uniform plan)
    const SpanPlan p = span_plan(B, T, halo, allowed);
    return p.nwgB ? p.nwgB : B;
}

// Variable-length batches: the lengths live on the device, so the plan cannot use them -- every workgroup of whole
// rounds of the chip takes an equal share of the frames that exist (prefix table from launch_len_prefix).
bool var_spans_usable(int B) { return B >= 1 && B <= PREF_MAX_B; }
static int var_span_workgroups(int B) { return 256 * ((B + 255) / 256); }
int launch_len_prefix(const int* lens, int B, int T, int* pref, hipStream_t s) {
    if (!var_spans_usable(B)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_len_prefix, dim3(1), dim3(PREF_MAX_B), 0, s, lens, B, T, pref);
    GT_LAUNCH_CHECK();
    return 0;
}

// 16-bit PCM at the host boundary.  The reference's data are mono 16-bit WAV files (infer.py:54, examples/*.wav) and its
// callers widen them on the host (soundfile / librosa); a caller that hands the SAMPLES over as int16 moves half the bytes
// over the host link, which is what bounds the served rate (bench.py io).  In: x = s / 32768 (exact in fp32: what
// soundfile.read returns).  Out: s = clip(rint(y * 32768), -32768, 32767), round half to even -- scipy.io.wavfile.write
// of np.rint(...), torch.round, and write_wav_pcm16 of gtcrn_micro_amd/infer.py all agree.  8 samples per lane and step.
typedef short i16x8 __attribute__((ext_vector_type(8)));
__global__ __launch_bounds__(256) void k_pcm16_to_f32(const i16x8* __restrict__ src, f32x4* __restrict__ dst, long n8) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
        const i16x8 v = __builtin_nontemporal_load(src + i);
        f32x4 a, b;
#pragma unroll
        for (int k = 0; k < 4; ++k) { a[k] = pcm16_widen(v[k]); b[k] = pcm16_widen(v[4 + k]); }
        dst[2 * i] = a;
        dst[2 * i + 1] = b;
    }
}
__global__ __launch_bounds__(256) void k_f32_to_pcm16(const f32x4* __restrict__ src, i16x8* __restrict__ dst, long n8) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
        const f32x4 a = __builtin_nontemporal_load(src + 2 * i), b = __builtin_nontemporal_load(src + 2 * i + 1);
        i16x8 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = (short)pcm16_round(a[k]);
            v[4 + k] = (short)pcm16_round(b[k]);
        }
        dst[i] = v;
    }
}
// n samples (a multiple of 8), both pointers 16-byte aligned; dir 0: int16 -> float32, 1: float32 -> int16
int launch_pcm16_convert(const void* src, void* dst, long n, int dir, hipStream_t s) {
    if (n <= 0 || (n & 7) || ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15)) return (int)hipErrorInvalidValue;
    const long n8 = n / 8;
    const int grid = (int)std::min<long>((n8 + 255) / 256, 256 * 16);
    if (dir == 0) hipLaunchKernelGGL(k_pcm16_to_f32, dim3(grid), dim3(256), 0, s, reinterpret_cast<const i16x8*>(src), reinterpret_cast<f32x4*>(dst), n8);
    else hipLaunchKernelGGL(k_f32_to_pcm16, dim3(grid), dim3(256), 0, s, reinterpret_cast<const f32x4*>(src), reinterpret_cast<i16x8*>(dst), n8);
    GT_LAUNCH_CHECK();
    return 0;
}

// G.711 at the host boundary, for the offline and hop-form caller (the packet forms take the codes themselves): one byte
// a sample over the host link.  In: x = D_law[c] / 32768 (exact).  Out: E_law(clip(rint(y * 32768))), the PCM16 rounding and
// then the integer map (kernels.h).  16 codes per lane and step: one 16-byte access on the byte side, four on the float side.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
template <int LAW>
__global__ __launch_bounds__(256) void k_g711_to_f32(const u32x4* __restrict__ src, f32x4* __restrict__ dst, long n16) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride) {
        const u32x4 v = __builtin_nontemporal_load(src + i);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            f32x4 a;
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] = pcm16_widen(g711_decode(LAW, (v[w] >> (8 * k)) & 0xFFu));
            dst[4 * i + w] = a;
        }
    }
}
template <int LAW>
__global__ __launch_bounds__(256) void k_f32_to_g711(const f32x4* __restrict__ src, u32x4* __restrict__ dst, long n16) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride) {
        u32x4 v;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const f32x4 a = __builtin_nontemporal_load(src + 4 * i + w);
            unsigned word = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) word |= g711_encode(LAW, pcm16_round(a[k])) << (8 * k);
            v[w] = word;
        }
        dst[i] = v;
    }
}
// n codes (a multiple of 16), both pointers 16-byte aligned; law 0 / 1; dir 0: codes -> float32, 1: float32 -> codes
int launch_g711_convert(const void* src, void* dst, long n, int law, int dir, hipStream_t s) {
    if (n <= 0 || (n & 15) || (law != 0 && law != 1) || (dir != 0 && dir != 1) ||
        ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15))
        return (int)hipErrorInvalidValue;
    const long n16 = n / 16;
    const int grid = (int)std::min<long>((n16 + 255) / 256, 256 * 16);
    if (dir == 0) {
        const u32x4* a = reinterpret_cast<const u32x4*>(src);
        f32x4* b = reinterpret_cast<f32x4*>(dst);
        if (law == 0) hipLaunchKernelGGL((k_g711_to_f32<0>), dim3(grid), dim3(256), 0, s, a, b, n16);
        else hipLaunchKernelGGL((k_g711_to_f32<1>), dim3(grid), dim3(256), 0, s, a, b, n16);
    } else {
        const f32x4* a = reinterpret_cast<const f32x4*>(src);
        u32x4* b = reinterpret_cast<u32x4*>(dst);
        if (law == 0) hipLaunchKernelGGL((k_f32_to_g711<0>), dim3(grid), dim3(256), 0, s, a, b, n16);
        else hipLaunchKernelGGL((k_f32_to_g711<1>), dim3(grid), dim3(256), 0, s, a, b, n16);
    }
    GT_LAUNCH_CHECK();
    return 0;
}

int launch_stft(const float* wave, int B, long L, int T, const int* lens, const float* win, const float* twid,
                float* spec, long sb, long sf, long st, float* frames, hipStream_t s) {
    const long nframes = (long)B * T;
    const int per = FFT_WAVES * FRAMES_PER_WAVE;
    const int grid = (int)((nframes + per - 1) / per);
    hipLaunchKernelGGL(k_stft<false>, dim3(grid), dim3(FFT_WAVES * 64), 0, s, wave, B, L, T, lens, win,
                       reinterpret_cast<const float2*>(twid), spec, sb, sf, st, frames);
    GT_LAUNCH_CHECK();
    return 0;
}

// calls f(std::bool_constant<...>{}...) with the run-time flags as compile-time values: one spelling of a launch serves
// every instantiation of its kernel template
template <bool... Bs, class F>
static void with_flags(F&& f) { f(std::bool_constant<Bs>{}...); }
template <bool... Bs, class F, class... R>
static void with_flags(F&& f, bool b, R... rest) {
    if (b) with_flags<Bs..., true>(f, rest...);
    else with_flags<Bs..., false>(f, rest...);
}
template <Synth M = Synth::Plain, class F, class... R>      // the same with a synthesis mode m in front of the flags
static void with_mode(F&& f, Synth m, R... flags) {
    if (m == M) with_flags([&](auto... bs) { f(std::integral_constant<Synth, M>{}, bs...); }, flags...);
    else if constexpr (M != Synth::Guard) with_mode<Synth((int)M + 1)>(f, m, flags...);
}

template <typename S>
int launch_wave_analysis(const S* in, long in_stride, int N, int nhops, int r, bool flush, const float* wstate,
                         const float* win, const float* twid, float* spec, Rows rows, hipStream_t s) {
    if (rows.slots && nhops != 1) return (int)hipErrorInvalidValue;
    const long nframes = (long)N * nhops;
    const int per = FFT_WAVES * WAVE_FRAMES;
    const int grid = (int)((nframes + per - 1) / per);
    const float2* tw = reinterpret_cast<const float2*>(twid);
    with_flags([&](auto FLUSH, auto IDX) {
        hipLaunchKernelGGL((k_wave_analysis<S, FLUSH.value, IDX.value>), dim3(grid), dim3(FFT_WAVES * 64), 0, s, in, in_stride, N,
                           flush ? 1 : nhops, flush ? r : 0, wstate, win, tw, spec, rows.slots, rows.cnt);
    }, flush, rows.slots != nullptr);
    GT_LAUNCH_CHECK();
    return 0;
}
template <typename S>
int launch_wave_synthesis(const float* spec, const S* in, long in_stride, S* out, long out_stride, int N, int nhops, int r,
                          bool flush, float* wstate, const float* win, const float* twid, Rows rows, WaveOpts o, hipStream_t s) {
    if (rows.slots && nhops != 1) return (int)hipErrorInvalidValue;
    const int grid = (N + FFT_WAVES - 1) / FFT_WAVES;
    const float2* tw = reinterpret_cast<const float2*>(twid);
    // a mixed flush with r == 0 may come without a tail pointer: its one block takes its dry samples from the ring alone
    with_mode([&](auto MODE, auto FLUSH, auto IDX) {
        hipLaunchKernelGGL((k_wave_synthesis<S, FLUSH.value, IDX.value, MODE.value>), dim3(grid), dim3(FFT_WAVES * 64), 0, s, spec,
                           in, in_stride, out, out_stride, N, flush ? 1 : nhops, flush ? r : 0, wstate, win, tw, o.gain, rows.slots,
                           rows.cnt, o.meters, o.ramp, o.alc, o.alc_params, o.tone, o.tone_params, o.tone_table);
    }, synth_mode(o), flush, rows.slots != nullptr);
    GT_LAUNCH_CHECK();
    return 0;
}
template int launch_wave_analysis<float>(const float*, long, int, int, int, bool, const float*, const float*, const float*, float*, Rows, hipStream_t);
template int launch_wave_analysis<short>(const short*, long, int, int, int, bool, const float*, const float*, const float*, float*, Rows, hipStream_t);
template int launch_wave_synthesis<float>(const float*, const float*, long, float*, long, int, int, int, bool, float*, const float*, const float*, Rows, WaveOpts, hipStream_t);
template int launch_wave_synthesis<short>(const float*, const short*, long, short*, long, int, int, int, bool, float*, const float*, const float*, Rows, WaveOpts, hipStream_t);

int launch_istft_adjoint(const float* gwave, int B, int T, const float* win, const float* twid, float* gspec, long sb,
                         long sf, long st, hipStream_t s) {
    const long nframes = (long)B * T;
    const int per = FFT_WAVES * FRAMES_PER_WAVE;
    const int grid = (int)((nframes + per - 1) / per);
    hipLaunchKernelGGL(k_stft<true>, dim3(grid), dim3(FFT_WAVES * 64), 0, s, gwave, B, 256L * (T - 1), T,
                       (const int*)nullptr, win,
                       reinterpret_cast<const float2*>(twid), gspec, sb, sf, st, (float*)nullptr);
    GT_LAUNCH_CHECK();
    return 0;
}

int launch_istft(const float* spec, long sb, long sf, long st, int B, int T, const int* lens, const float* win,
                 const float* twid, float* wave, hipStream_t s, const float* dry, long dry_stride, const float* gain) {
    const int groups = (T - 1 + ISTFT_BLOCKS - 1) / ISTFT_BLOCKS;
    if (gain) hipLaunchKernelGGL(k_istft_mix, dim3(B * groups), dim3(FFT_WAVES * 64), 0, s, spec, sb, sf, st, B, T, lens, win,
                                 reinterpret_cast<const float2*>(twid), wave, dry, dry_stride, gain);
    else hipLaunchKernelGGL(k_istft, dim3(B * groups), dim3(FFT_WAVES * 64), 0, s, spec, sb, sf, st, B, T, lens, win,
                            reinterpret_cast<const float2*>(twid), wave);
    GT_LAUNCH_CHECK();
    return 0;
}

int configure_kernels() {
    hipError_t e;
    const void* enc[] = {reinterpret_cast<const void*>(k_encoder<TPW, false, false, false, true>),
                         reinterpret_cast<const void*>(k_encoder<TPW, false, false, true>),
                         reinterpret_cast<const void*>(k_encoder<1, false, false, true>),
                         reinterpret_cast<const void*>(k_encoder<2, false, false, true>),
                         reinterpret_cast<const void*>(k_encoder<TPW, false, false, false>),
                         reinterpret_cast<const void*>(k_encoder<1, false, false, false>),
                         reinterpret_cast<const void*>(k_encoder<2, false, false, false>),
                         reinterpret_cast<const void*>(k_encoder<TPW, false, true, false>)};
    const void* fr[] = {reinterpret_cast<const void*>(k_front<true, false>), reinterpret_cast<const void*>(k_front<false, false>),
                        reinterpret_cast<const void*>(k_front<true, true>), reinterpret_cast<const void*>(k_front<false, true>)};
    for (const void* f : fr) {
        e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, FR_LDS_FLOATS * 4);
        if (e != hipSuccess) return (int)e;
    }
    for (const void* f : enc) {
        e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, max(ENC_LDS_FLOATS, ENC_GT_LDS_FLOATS) * 4);
        if (e != hipSuccess) return (int)e;
    }
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_encoder<1, true, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            ENC_MS_LDS_FLOATS * 4);
    if (e != hipSuccess) return (int)e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_decoder<false, 1, true, false>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, DEC_MS_LDS_FLOATS * 4);
    if (e != hipSuccess) return (int)e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_stream_ms), hipFuncAttributeMaxDynamicSharedMemorySize,
                            SM_LDS_FLOATS * 4);
    if (e != hipSuccess) return (int)e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_stream_wide<SwCfg>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            SW_LDS_FLOATS * 4);
    if (e != hipSuccess) return (int)e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_stream_ms_slots), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (SM_LDS_FLOATS + SLOT_WORDS) * 4);
    if (e != hipSuccess) return (int)e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_stream_wide<SwCfg, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (SW_LDS_FLOATS + SLOT_WORDS) * 4);
    if (e != hipSuccess) return (int)e;
    const void* gt[] = {reinterpret_cast<const void*>(k_gtcn<TPW, false>), reinterpret_cast<const void*>(k_gtcn<1, false>),
                        reinterpret_cast<const void*>(k_gtcn<1, true>),
                        reinterpret_cast<const void*>(k_gtcn<2, true>), reinterpret_cast<const void*>(k_gtcn<2, false>)};
    for (const void* f : gt) {
        e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, GT_LDS_FLOATS * 4);
        if (e != hipSuccess) return (int)e;
    }
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_gtcn_band<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            GB_LDS_FLOATS * 4);
    if (e != hipSuccess) return (int)e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_gtcn_band<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            GB_LDS_FLOATS * 4);
    if (e != hipSuccess) return (int)e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_gtcn_band<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            GB_LDS_FLOATS * 4);
    if (e != hipSuccess) return (int)e;
    const void* dec[] = {reinterpret_cast<const void*>(k_decoder<false, TPW, false, false, true>),
                         reinterpret_cast<const void*>(k_decoder<true, TPW, false, false, true>),
                         reinterpret_cast<const void*>(k_decoder<false, TPW, false, false>),
                         reinterpret_cast<const void*>(k_decoder<true, TPW, false, false>),
                         reinterpret_cast<const void*>(k_decoder<false, 1, false, false>),
                         reinterpret_cast<const void*>(k_decoder<true, 1, false, false>),
                         reinterpret_cast<const void*>(k_decoder<false, 2, false, false>),
                         reinterpret_cast<const void*>(k_decoder<true, 2, false, false>),
                         reinterpret_cast<const void*>(k_decoder<false, TPW, false, true>),
                         reinterpret_cast<const void*>(k_decoder<true, TPW, false, true>)};
    for (const void* f : dec) {
        e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, DEC_LDS_FLOATS * 4);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

// the multi-stream form serves single-frame streaming steps: one new frame for each of B streams
static bool use_multi_stream(int T, const float* state, long sb) {
    return state != nullptr && T == 1 && (MS_ROWS - 1) * (sb < 0 ? -sb : sb) < (1L << 31);
}

// The offline front end (see k_front): frames from a waveform (wave != nullptr: STFT fused, the spectrogram is also
// written frame-major to `spec_out`) or from a caller spectrogram (spec_in, strides).  Persistent grid.
int launch_front(const float* wave, long L, const float* spec_in, long isb, long isf, long ist, int B, int T,
                 const int* lens, const float* win, const float* twid, const float* PF, const int* PI, float* spec_out,
                 float* en0, float* en1p, hipStream_t s, const Quant* q) {
    const long wgs = ((long)B * T + FR_WAVES - 1) / FR_WAVES;
    const int grid = (int)(wgs < 256 * 2 ? wgs : 256 * 2);              // two workgroups per CU, persistent
    const float qin = q ? q->in_step : 0.f;
    const float2* tw = reinterpret_cast<const float2*>(twid);
#define GT_FRONT(WV, QV, INP)                                                                                      \
    hipLaunchKernelGGL((k_front<WV, QV>), dim3(grid), dim3(FR_NT), FR_LDS_FLOATS * 4, s, INP, L, isb, isf, ist, B, T, \
                       lens, win, tw, PF, PI, spec_out, en0, en1p, qin)
    if (wave) { if (q) GT_FRONT(true, true, wave); else GT_FRONT(true, false, wave); }
    else { if (q) GT_FRONT(false, true, spec_in); else GT_FRONT(false, false, spec_in); }
#undef GT_FRONT
    GT_LAUNCH_CHECK();
    return 0;
}

// front_done: k_front has produced en0 / en1 already, only the three GTConv blocks run here (offline calls)
int launch_encoder(const float* spec, long sb, long sf, long st, int B, int T, const int* lens, const float* PF,
                   const int* PI, float* en0, float* en1, float* en2, float* en3, float* en4, float* state,
                   unsigned long long* stamps, hipStream_t s, const Quant* q, bool front_done, const int* pref) {
    // offline fp32 blocks-only form: the workgroups may share the (utterance, frame) axis (span_begin, SPANS instantiation)
    const SpanPlan pl = span_plan(B, T, HALO_BLOCKS, front_done && !state && !q && lens == nullptr);
    if (pref && front_done && !state && !q) {          // variable-length batch in shares (pref: see launch_len_prefix)
        hipLaunchKernelGGL((k_encoder<TPW, false, false, false, true>), dim3(var_span_workgroups(B)), dim3(NTHR),
                           ENC_GT_LDS_FLOATS * 4, s, spec, sb, sf, st, T, pref, B, 0.f, PF, PI, en0, en1, en2, en3, en4, state,
                           stamps);
        GT_LAUNCH_CHECK();
        return 0;
    }
#define GT_ENC(TPWV, QV, FRV)                                                                                       \
    hipLaunchKernelGGL((k_encoder<TPWV, false, QV, FRV>), dim3(B), dim3(NTHR),                                      \
                       (FRV ? ENC_LDS_FLOATS : ENC_GT_LDS_FLOATS) * 4, s, spec, sb, sf, st,                         \
                       T, lens, B, q ? q->in_step : 0.f, PF, PI, en0, en1, en2, en3, en4, state, stamps)
    if (q) {   // int8-weight / fp16-activation variant: offline form only, the full-chunk instantiation
        if (!front_done || state) return (int)hipErrorInvalidValue;
        GT_ENC(TPW, true, false);
    } else if (use_multi_stream(T, state, sb)) {
        // streams b*4 .. b*4+3 become rows 0..3 of workgroup b: sb' = 4 sb, st' = sb, T' = 4
        const int grid = (B + MS_STREAMS - 1) / MS_STREAMS;
        hipLaunchKernelGGL((k_encoder<1, true, false, true>), dim3(grid), dim3(NTHR), ENC_MS_LDS_FLOATS * 4, s, spec,
                           (long)MS_STREAMS * sb, sf, sb, MS_STREAMS, (const int*)nullptr, B, 0.f, PF, PI, en0, en1, en2, en3, en4, state, stamps);
    } else if (front_done && pl.nwgB) {
        // (the blocks-only form reads en1 and writes en2 .. en4; the spectrogram and en0 are not touched)
        if (pl.nA)
            hipLaunchKernelGGL((k_encoder<TPW, false, false, false>), dim3(pl.nA), dim3(NTHR), ENC_GT_LDS_FLOATS * 4, s, spec,
                               sb, sf, st, T, lens, pl.nA, 0.f, PF, PI, en0, en1, en2, en3, en4, state, stamps);
        const long o = (long)pl.nA * T * 528;
        hipLaunchKernelGGL((k_encoder<TPW, false, false, false, true>), dim3(pl.nwgB), dim3(NTHR), ENC_GT_LDS_FLOATS * 4, s,
                           spec, sb, sf, st, T, lens, B - pl.nA, 0.f, PF, PI, en0, en1 + o, en2 + o, en3 + o, en4 + o, state,
                           stamps ? stamps + (long)pl.nA * 16 : nullptr);     // (its stamp rows behind the first launch's)
    } else if (front_done) {
        if (T <= SHORT_T) GT_ENC(1, false, false);
        else if (T <= SHORT_T2) GT_ENC(2, false, false);
        else GT_ENC(TPW, false, false);
    } else {
        if (T <= SHORT_T) GT_ENC(1, false, true);
        else if (T <= SHORT_T2) GT_ENC(2, false, true);
        else GT_ENC(TPW, false, true);
    }
#undef GT_ENC
    GT_LAUNCH_CHECK();
    return 0;
}

int launch_gtcn(const float* xin, float* xout, const float* P, int B, int T, float* state, int st_off,
                const float* addend, unsigned long long* stamps, hipStream_t s) {
    if (T <= SHORT_T && state)   // streaming step: rings stay in the stream state (no LDS copy: 77 KB, 2 workgroups per CU)
        hipLaunchKernelGGL((k_gtcn<1, true>), dim3(B), dim3(NTHR), GT_LDS_H * 4, s, xin, xout, P, T, state, st_off,
                           addend, stamps);
    else if (T <= SHORT_T)
        hipLaunchKernelGGL((k_gtcn<1, false>), dim3(B), dim3(NTHR), GT_LDS_FLOATS * 4, s, xin, xout, P, T, state,
                           st_off, addend, stamps);
    else if (T <= SHORT_T2 && state)
        hipLaunchKernelGGL((k_gtcn<2, true>), dim3(B), dim3(NTHR), GT_LDS_H * 4, s, xin, xout, P, T, state, st_off,
                           addend, stamps);
    else if (T <= SHORT_T2)
        hipLaunchKernelGGL((k_gtcn<2, false>), dim3(B), dim3(NTHR), GT_LDS_FLOATS * 4, s, xin, xout, P, T, state,
                           st_off, addend, stamps);
    else   // (11..16-frame stateful calls take the LDS-ring form too: the in-state form with three tiles per wave spilled)
        hipLaunchKernelGGL((k_gtcn<TPW, false>), dim3(B), dim3(NTHR), GT_LDS_FLOATS * 4, s, xin, xout, P, T, state,
                           st_off, addend, stamps);
    GT_LAUNCH_CHECK();
    return 0;
}

// single-frame step for B streams: BOTH GTCN stacks, per position, barrier-free (see k_gtcn_ms); P = the two stacks'
// parameters back to back
int launch_gtcn_ms(const float* xin, float* xout1, float* xout2, const float* P, int B, float* state, hipStream_t s) {
    const long tiles = ((long)B * 33 + 15) / 16;
    hipLaunchKernelGGL(k_gtcn_ms, dim3((unsigned)((tiles + GTMS_WAVES - 1) / GTMS_WAVES)), dim3(GTMS_WAVES * 64), 0, s, xin,
                       xout1, xout2, P, B, state);
    GT_LAUNCH_CHECK();
    return 0;
}

int launch_gtcn_band(const float* xin, float* xout, const float* P, int B, int T, const int* lens, const float* addend,
                     hipStream_t s, const Quant* q, const int* pref) {
    if (pref && !q) {
        hipLaunchKernelGGL((k_gtcn_band<false, true>), dim3(var_span_workgroups(B)), dim3(NTHR), GB_LDS_FLOATS * 4, s, xin, xout,
                           P, B, T, pref, addend);
        GT_LAUNCH_CHECK();
        return 0;
    }
    if (q) {
        hipLaunchKernelGGL(k_gtcn_band<true>, dim3(B), dim3(NTHR), GB_LDS_FLOATS * 4, s, xin, xout, P, B, T, lens, addend);
        GT_LAUNCH_CHECK();
        return 0;
    }
    const SpanPlan pl = span_plan(B, T, HALO_GTCN, lens == nullptr);
    if (pl.nA)
        hipLaunchKernelGGL(k_gtcn_band<false>, dim3(pl.nA), dim3(NTHR), GB_LDS_FLOATS * 4, s, xin, xout, P, pl.nA, T, lens,
                           addend);
    if (pl.nwgB) {
        const long o = (long)pl.nA * T * 528;
        hipLaunchKernelGGL((k_gtcn_band<false, true>), dim3(pl.nwgB), dim3(NTHR), GB_LDS_FLOATS * 4, s, xin + o, xout + o, P,
                           B - pl.nA, T, lens, addend ? addend + o : nullptr);
    }
    GT_LAUNCH_CHECK();
    return 0;
}

int launch_decoder(const float* xg, const float* en0, const float* en1, const float* en2, const float* en3,
                   const float* en4, const float* spec, long sb, long sf, long st, float* out, long osb, long osf,
                   long ost, int B, int T, const int* lens, const float* PF, const int* PI, float* state, float* dbg,
                   unsigned long long* stamps, hipStream_t s, const Quant* q, const int* pref) {
    if (pref && !state && !q) {                        // variable-length batch in shares (pref: see launch_len_prefix)
        const int nwg = var_span_workgroups(B);
        if (dbg)
            hipLaunchKernelGGL((k_decoder<true, TPW, false, false, true>), dim3(nwg), dim3(NTHR), DEC_LDS_FLOATS * 4, s, xg, en0,
                               en1, en2, en3, en4, spec, sb, sf, st, out, osb, osf, ost, T, pref, B, 0.f, 0.f, PF, PI, state, dbg,
                               stamps);
        else
            hipLaunchKernelGGL((k_decoder<false, TPW, false, false, true>), dim3(nwg), dim3(NTHR), DEC_LDS_FLOATS * 4, s, xg, en0,
                               en1, en2, en3, en4, spec, sb, sf, st, out, osb, osf, ost, T, pref, B, 0.f, 0.f, PF, PI, state, dbg,
                               stamps);
        GT_LAUNCH_CHECK();
        return 0;
    }
    // offline fp32 calls: the workgroups may share the (utterance, frame) axis (span_begin, SPANS instantiation); the stage
    // taps (dbg) index by the batch position, so a debug run is never split into two launches
    SpanPlan pl = span_plan(B, T, HALO_BLOCKS, !state && !q && lens == nullptr);
    if (dbg && pl.nA && pl.nwgB) {
        long c = 0;
        pl = SpanPlan{0, best_spans(B, T, HALO_BLOCKS, &c)};
        if (!pl.nwgB) pl = SpanPlan{B, 0};
    }
#define GT_DEC(DBGV, TPWV)                                                                                         \
    hipLaunchKernelGGL((k_decoder<DBGV, TPWV, false, false>), dim3(B), dim3(NTHR), DEC_LDS_FLOATS * 4, s, xg, en0, en1, \
                       en2, en3, en4, spec, sb, sf, st, out, osb, osf, ost, T, lens, B, 0.f, 0.f, PF, PI, state, dbg,   \
                       stamps)
    if (q) {
        // (dbg: the stage-tap instantiation, de0..de4 as fp32 copies of the fp16-valued registers)
        if (dbg)
            hipLaunchKernelGGL((k_decoder<true, TPW, false, true>), dim3(B), dim3(NTHR), DEC_LDS_FLOATS * 4, s, xg, en0, en1,
                               en2, en3, en4, spec, sb, sf, st, out, osb, osf, ost, T, lens, B, q->in_step, q->out_step, PF,
                               PI, (float*)nullptr, dbg, stamps);
        else
            hipLaunchKernelGGL((k_decoder<false, TPW, false, true>), dim3(B), dim3(NTHR), DEC_LDS_FLOATS * 4, s, xg, en0, en1,
                               en2, en3, en4, spec, sb, sf, st, out, osb, osf, ost, T, lens, B, q->in_step, q->out_step, PF,
                               PI, (float*)nullptr, (float*)nullptr, stamps);
    } else if (!dbg && use_multi_stream(T, state, sb) && use_multi_stream(T, state, osb)) {
        const int grid = (B + MS_STREAMS - 1) / MS_STREAMS;
        hipLaunchKernelGGL((k_decoder<false, 1, true, false>), dim3(grid), dim3(NTHR), DEC_MS_LDS_FLOATS * 4, s, xg, en0,
                           en1, en2, en3, en4, spec, (long)MS_STREAMS * sb, sf, sb, out, (long)MS_STREAMS * osb, osf, osb,
                           MS_STREAMS, (const int*)nullptr, B, 0.f, 0.f, PF, PI, state, (float*)nullptr, stamps);
    } else if (pl.nwgB) {
        if (pl.nA)
            hipLaunchKernelGGL((k_decoder<false, TPW, false, false>), dim3(pl.nA), dim3(NTHR), DEC_LDS_FLOATS * 4, s, xg, en0,
                               en1, en2, en3, en4, spec, sb, sf, st, out, osb, osf, ost, T, lens, pl.nA, 0.f, 0.f, PF, PI,
                               state, dbg, stamps);
        const long o = (long)pl.nA * T * 528, o0 = (long)pl.nA * T * (F1 * 16);
        const float* specB = spec + (long)pl.nA * sb;
        float* outB = out + (long)pl.nA * osb;
        if (dbg)
            hipLaunchKernelGGL((k_decoder<true, TPW, false, false, true>), dim3(pl.nwgB), dim3(NTHR), DEC_LDS_FLOATS * 4, s,
                               xg + o, en0 + o0, en1 + o, en2 + o, en3 + o, en4 + o, specB, sb, sf, st, outB, osb, osf, ost, T,
                               lens, B - pl.nA, 0.f, 0.f, PF, PI, state, dbg, stamps ? stamps + (long)pl.nA * 16 : nullptr);
        else
            hipLaunchKernelGGL((k_decoder<false, TPW, false, false, true>), dim3(pl.nwgB), dim3(NTHR), DEC_LDS_FLOATS * 4, s,
                               xg + o, en0 + o0, en1 + o, en2 + o, en3 + o, en4 + o, specB, sb, sf, st, outB, osb, osf, ost, T,
                               lens, B - pl.nA, 0.f, 0.f, PF, PI, state, dbg, stamps ? stamps + (long)pl.nA * 16 : nullptr);
    } else if (T <= SHORT_T) {
        if (dbg) GT_DEC(true, 1); else GT_DEC(false, 1);
    } else if (T <= SHORT_T2) {
        if (dbg) GT_DEC(true, 2); else GT_DEC(false, 2);
    } else {
        if (dbg) GT_DEC(true, TPW); else GT_DEC(false, TPW);
    }
#undef GT_DEC
    GT_LAUNCH_CHECK();
    return 0;
}

// (GTCRN_STAGGER = "phases,unit" overrides the default for measurements: tools/stream_form_ab.py)
static int stagger_setting() {
    static const int v = [] {
        int ph = 32, unit = 5;
        if (const char* e = getenv("GTCRN_STAGGER")) {
            if (sscanf(e, "%d,%d", &ph, &unit) != 2 || ph < 1 || ph > 256 || (ph & (ph - 1)) || unit < 0 || unit > 255) { ph = 32; unit = 5; }
        }
        return unit == 0 ? 0 : (ph << 8) | unit;
    }();
    return v;
}
// single-frame step for B streams (rows.slots: max_active rows), ONE launch: the narrow form (k_stream_ms / k_stream_ms_slots,
// MS_STREAMS streams per workgroup) or the wide one (k_stream_wide, SwCfg::NS); strides in floats of (B,257,1,2)-shaped tensors.
// The indexed kernels keep their workgroup's slot ids in SLOT_WORDS more LDS words.
int launch_stream_step(bool wide, const float* spec, long sb, long sf, float* out, long osb, long osf, int B, const float* PF,
                       const int* PI, float* state, unsigned long long* stamps, Rows rows, hipStream_t s) {
    const int per = wide ? SwCfg::NS : MS_STREAMS, grid = (B + per - 1) / per;
    const size_t slot_lds = rows.slots ? SLOT_WORDS * 4 : 0;
    if (wide) {
        // from three rounds of workgroups on: 32 start shifts of 5 x 512 clocks (two thirds of a ~118 k-cycle workgroup in all;
        // swept on the GPU, tools/stagger_sweep.sh -> profiles/r06_ab_stream_wide.txt)
        const int stagger = grid >= 3 * 256 ? stagger_setting() : 0;
        with_flags([&](auto IDX) {
            hipLaunchKernelGGL((k_stream_wide<SwCfg, IDX.value>), dim3(grid), dim3(SwCfg::NT), SW_LDS_FLOATS * 4 + slot_lds, s, spec, sb,
                               sf, out, osb, osf, B, PF, PI, state, stamps, stagger, rows.slots, rows.cnt);
        }, rows.slots != nullptr);
    } else if (rows.slots) {
        hipLaunchKernelGGL(k_stream_ms_slots, dim3(grid), dim3(NTHR), SM_LDS_FLOATS * 4 + slot_lds, s, spec, sb, sf, out, osb, osf, B,
                           PF, PI, state, stamps, 0, rows.slots, rows.cnt);
    } else {
        // no stagger: measured, no gain for this form, and the first round's sleeps cost 20 % at four rounds
        hipLaunchKernelGGL(k_stream_ms, dim3(grid), dim3(NTHR), SM_LDS_FLOATS * 4, s, spec, sb, sf, out, osb, osf, B, PF, PI,
                           state, stamps, 0);
    }
    GT_LAUNCH_CHECK();
    return 0;
}
int launch_reset_slots(float* state, float* wstate, const int* slots, const int* cnt, int max_active, hipStream_t s) {
    hipLaunchKernelGGL(k_reset_slots, dim3(max_active, RESET_PARTS), dim3(256), 0, s, state, wstate, slots, cnt, max_active);
    GT_LAUNCH_CHECK();
    return 0;
}
int stream_wide_streams() { return SwCfg::NS; }

bool stream_ms_usable(long sb, long osb) {
    const long a = sb < 0 ? -sb : sb, o = osb < 0 ? -osb : osb;
    return 8 * a < (1L << 31) && 8 * o < (1L << 31);     // (row offsets of either form in 32 bits)
}

int launch_state_convert(float* state, int N, float* conv, float* tra, float* const* tcn8, const int* PI, int dir,
                         hipStream_t s) {
    hipLaunchKernelGGL(k_state_convert, dim3(N), dim3(256), 0, s, state, N, conv, tra, tcn8, PI, dir);
    GT_LAUNCH_CHECK();
    return 0;
}

int launch_conv2d_causal(const float* x, const float* cache, const float* w, const float* bias, float* y,
                         float* cache_out, int B, int Cin, int Cout, int T, int F, int kt, int kf, int dt, int df,
                         int pf, int groups, int transposed, int Fout, hipStream_t s) {
    const long total = (long)B * Cout * T * Fout;
    const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_conv2d_causal, dim3(grid > 0 ? grid : 1), dim3(256), 0, s, x, cache, w, bias, y, cache_out, B,
                       Cin, Cout, T, F, kt, kf, dt, df, pf, groups, transposed, Fout);
    GT_LAUNCH_CHECK();
    return 0;
}

int launch_selftest_split3(const float* x, long n, float* planes, float* joined, const float* A, const float* Bm,
                           float* D, hipStream_t s) {
    hipLaunchKernelGGL(k_selftest_split3, dim3(64), dim3(256), 0, s, x, n, planes, joined, A, Bm, D);
    GT_LAUNCH_CHECK();
    return 0;
}

int launch_selftest(const float* A, const float* Bm, const float* C, float* D, hipStream_t s) {
    hipLaunchKernelGGL(k_selftest, dim3(1), dim3(64), 0, s, A, Bm, C, D);
    GT_LAUNCH_CHECK();
    return 0;
}

// ===================================================================== sample-rate conversion (gtcrn_resample, gtcrn_rate_stream_*)
// Polyphase FIR between 16 kHz and the caller's rate (include/gtcrn_micro_hip.h: the filter is designed on the host).  The
// taps arrive as a phase table P[k0][t] = h[k0 + t * up] (k0 < up, t < ntp; ntp = the taps of the longest phase rounded up
// to a multiple of 4, the rest +0.0f), so output j of  y[j] = sum_i x[i] h[j down - i up + half]  is the dot product of
// row k0 = (j down + half) mod up with the samples x[ihi], x[ihi - 1], ..., ihi = (j down + half) div up.
//
// rs_dot is that dot product and the ONLY place a sample meets a tap: ntp products in the table's order into four fp32
// accumulators (tap t into accumulator t mod 4) by fmaf, joined (a0 + a1) + (a2 + a3).  Samples outside the signal are
// staged as +0.0f and multiplied like any other.  The batch kernel and the two per-stream causal kernels stage the same
// sample values around the same expression, so a stream equals the batch call on the same signal bit for bit.
//
// A padding tap reads NO sample.  Every phase holds the longest phase's taps or one fewer, so a row ends in at most four
// +0.0f, all of them in its last group of four; a designed tap is never zero (gtcrn_resample_taps; the tests assert it for
// every supported pair).  0 * x is 0 only for a finite x: multiplied like the rest, a NaN or Inf sample would meet up to
// four padding taps in each of the `up` phases and so reach up to 4 * up outputs the filter's definition does not connect
// it with (3 + 4 + 4 = 11 at 16 -> 48 kHz).  So the last group selects the sample away (+0.0f, which the product would
// have been) where the tap's word is zero -- an integer compare, nothing -fno-honor-nans can reason about.
__device__ __forceinline__ float rs_pad(float h, float x) { return __float_as_uint(h) ? x : 0.f; }
__device__ __forceinline__ float rs_dot(const float* __restrict__ tp, int ntp, const float* __restrict__ xs) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    const int last = ntp - 4;
    for (int t = 0; t < last; t += 4) {
        const f32x4 h = ld4(tp + t);
        a0 = fmaf(h[0], xs[-t], a0);
        a1 = fmaf(h[1], xs[-t - 1], a1);
        a2 = fmaf(h[2], xs[-t - 2], a2);
        a3 = fmaf(h[3], xs[-t - 3], a3);
    }
    const f32x4 h = ld4(tp + last);
    a0 = fmaf(h[0], rs_pad(h[0], xs[-last]), a0);
    a1 = fmaf(h[1], rs_pad(h[1], xs[-last - 1]), a1);
    a2 = fmaf(h[2], rs_pad(h[2], xs[-last - 2]), a2);
    a3 = fmaf(h[3], rs_pad(h[3], xs[-last - 3]), a3);
    return (a0 + a1) + (a2 + a3);
}

// phase tables of at most RS_LDS_TAPS floats are staged in LDS (every integer ratio and 2/3, 3/2: <= 196 floats); the
// 147- to 640-phase tables of the 44.1 kHz family (57 - 164 KB) are read from global memory (L2)
__device__ __forceinline__ const float* rs_stage_taps(const float* __restrict__ taps, int n, float* s_t, int tid, int nthr) {
    if (n > RS_LDS_TAPS) return nullptr;
    for (int i = tid; i < n; i += nthr) s_t[i] = taps[i];
    return s_t;
}

// Batch form: a workgroup computes RS_TILE consecutive outputs of one row from the input span they read, staged once in
// LDS as floats (16-byte loads where the row allows it; +0.0f outside [0, row length)).  Lane j reads the samples
// around j * down / up: a stride of down / up <= 3 words between lanes -- 1 (up-sampling: neighbours share a word,
// broadcast), 3 (48 -> 16 kHz: conflict free on the 32 banks of ds_read_b32) or 2 (32 -> 16 kHz: two-way).
// Rows have their own lengths (lens, device; nullptr: all L); outputs beyond ceil(len * up / down) are not written.
template <typename SI, typename SO>
__global__ __launch_bounds__(RS_THREADS) void k_resample(const SI* __restrict__ in, long in_stride, const int* __restrict__ lens,
                                                         long L, SO* __restrict__ out, long out_stride, int tiles, int up,
                                                         int down, int half, int ntp, const float* __restrict__ taps, int vec) {
    __shared__ __attribute__((aligned(16))) float s_x[RS_SPAN];
    __shared__ __attribute__((aligned(16))) float s_t[RS_LDS_TAPS];
    const int tid = threadIdx.x;
    const int row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
    long len = lens ? (long)lens[row] : L;
    len = len < 0 ? 0 : (len > L ? L : len);
    const long nout = (len * up + down - 1) / down;
    const long j0 = (long)tile * RS_TILE;
    if (j0 >= nout) return;                                         // (workgroup uniform)
    const long j1 = j0 + RS_TILE < nout ? j0 + RS_TILE : nout;
    const float* tp = rs_stage_taps(taps, up * ntp, s_t, tid, RS_THREADS);
    constexpr int V = std::is_same<SI, short>::value ? 8 : 4;        // samples per 16-byte load
    const long lo = (j0 * down + half) / up - (ntp - 1), hi = ((j1 - 1) * down + half) / up;
    const long a0 = lo - (((lo % V) + V) % V);                     // the span starts on a 16-byte boundary of the row
    const int nv = (int)((hi - a0) / V) + 1;                       // nv * V <= RS_SPAN: launch_resample checks the worst tile
    const SI* x = in + (long)row * in_stride;
    for (int v = tid; v < nv; v += RS_THREADS) {
        const long i = a0 + (long)v * V;
        float f[V];
        if (vec && i >= 0 && i + V <= len) {
            if constexpr (V == 8) {
                const i16x8 q = *reinterpret_cast<const i16x8*>(x + i);
#pragma unroll
                for (int e = 0; e < 8; ++e) { const short qe = q[e]; f[e] = wave_ld<short>(&qe); }
            } else {
                const f32x4 q = *reinterpret_cast<const f32x4*>(x + i);
#pragma unroll
                for (int e = 0; e < 4; ++e) f[e] = q[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) f[e] = (i + e >= 0 && i + e < len) ? wave_ld<SI>(x + i + e) : 0.f;
        }
#pragma unroll
        for (int e = 0; e < V; e += 4) st4(s_x + v * V + e, f32x4{f[e], f[e + 1], f[e + 2], f[e + 3]});
    }
    __syncthreads();
    SO* o = out + (long)row * out_stride;
    for (long j = j0 + tid; j < j1; j += RS_THREADS) {
        const long num = j * down + half, ih = num / up;
        const int k0 = (int)(num - ih * up);
        const float* xs = s_x + (ih - a0);
        const float y = tp ? rs_dot(tp + k0 * ntp, ntp, xs) : rs_dot(taps + (long)k0 * ntp, ntp, xs);
        wave_st<SO>(o + j, y);
    }
}

// Per-stream causal form, one workgroup per stream: the stream's centred filter delayed by half / down output samples,
// so output m of a hop reads inputs up to (m down) div up of the SAME hop (hin * up == hout * down: every hop starts at
// phase 0) and back ntp - 1 samples, the first of which are the stream's history hist[0 .. ntp) (the last ntp input
// samples as floats; zeros after a reset).  Hop by hop: [previous ntp samples ++ the hop] staged in LDS, hout outputs,
// then the history advances to the call's last ntp input samples (ntp <= hin).
template <typename SI, typename SO>
__device__ __forceinline__ void rate_hops(const SI* __restrict__ x, SO* __restrict__ o, float* __restrict__ hist, int nhops,
                                          int hin, int hout, int up, int down, int ntp, const float* __restrict__ taps) {
    __shared__ __attribute__((aligned(16))) float s_x[RATE_SPAN];
    __shared__ __attribute__((aligned(16))) float s_t[RS_LDS_TAPS];
    const int tid = threadIdx.x;
    const float* tp = rs_stage_taps(taps, up * ntp, s_t, tid, RS_THREADS);      // (never nullptr: launch_rate checks)
    for (int h = 0; h < nhops; ++h) {
        for (int i = tid; i < ntp + hin; i += RS_THREADS) {
            const long g = (long)h * hin + i - ntp;
            s_x[i] = g >= 0 ? wave_ld<SI>(x + g) : hist[ntp + g];
        }
        __syncthreads();
        for (int m = tid; m < hout; m += RS_THREADS) {
            const int num = m * down, ih = num / up, k0 = num - ih * up;
            wave_st<SO>(o + (long)h * hout + m, rs_dot(tp + k0 * ntp, ntp, s_x + ntp + ih));
        }
        __syncthreads();
    }
    for (int i = tid; i < ntp; i += RS_THREADS) hist[i] = wave_ld<SI>(x + (long)nhops * hin - ntp + i);
}
// caller's rate -> 16 kHz in front of the wave step: rstate row = [inbound history | outbound history]
template <typename S>
__global__ __launch_bounds__(RS_THREADS) void k_rate_in(const S* __restrict__ in, long in_stride, float* __restrict__ out,
                                                        long out_stride, float* __restrict__ rstate, long rs_stride, int nhops,
                                                        int hin, int up, int down, int ntp, const float* __restrict__ taps) {
    const long n = blockIdx.x;
    rate_hops<S, float>(in + n * in_stride, out + n * out_stride, rstate + n * rs_stride, nhops, hin, 256, up, down, ntp, taps);
}
// 16 kHz -> caller's rate behind it, from the 256-sample blocks k_wave_synthesis emits
template <typename S>
__global__ __launch_bounds__(RS_THREADS) void k_rate_out(const float* __restrict__ in, long in_stride, S* __restrict__ out,
                                                         long out_stride, float* __restrict__ rstate, long rs_stride, int nhops,
                                                         int hout, int up, int down, int ntp, const float* __restrict__ taps) {
    const long n = blockIdx.x;
    rate_hops<float, S>(in + n * in_stride, out + n * out_stride, rstate + n * rs_stride, nhops, 256, hout, up, down, ntp, taps);
}

// the widest input span one tile of RS_TILE outputs stages (with the alignment slack of the 16-byte loads)
long resample_tile_span(int up, int down, int ntp) { return ((long)(RS_TILE - 1) * down + up - 1) / up + 1 + ntp + 8 + 8; }

template <typename SI, typename SO>
int launch_resample(const SI* in, long in_stride, const int* lens, long L, SO* out, long out_stride, int B, int up, int down,
                    int half, int ntp, const float* taps, hipStream_t s) {
    if (resample_tile_span(up, down, ntp) > RS_SPAN || (ntp & 3) || (reinterpret_cast<uintptr_t>(taps) & 15))
        return (int)hipErrorInvalidValue;
    const long nout = (L * up + down - 1) / down;
    const long tiles = (nout + RS_TILE - 1) / RS_TILE;
    if (tiles < 1 || tiles * B > 0x7fffffffL) return (int)hipErrorInvalidValue;
    constexpr int V = std::is_same<SI, short>::value ? 8 : 4;
    const int vec = !(reinterpret_cast<uintptr_t>(in) & 15) && in_stride % V == 0;
    hipLaunchKernelGGL((k_resample<SI, SO>), dim3((unsigned)(tiles * B)), dim3(RS_THREADS), 0, s, in, in_stride, lens, L, out,
                       out_stride, (int)tiles, up, down, half, ntp, taps, vec);
    GT_LAUNCH_CHECK();
    return 0;
}
template int launch_resample<float, float>(const float*, long, const int*, long, float*, long, int, int, int, int, int, const float*, hipStream_t);
template int launch_resample<short, float>(const short*, long, const int*, long, float*, long, int, int, int, int, int, const float*, hipStream_t);
template int launch_resample<float, short>(const float*, long, const int*, long, short*, long, int, int, int, int, int, const float*, hipStream_t);

static bool rate_geometry_ok(int hin, int hout, int up, int down, int ntp) {
    return (long)hin * up == (long)hout * down && ntp <= hin && !(ntp & 3) && ntp + hin <= RATE_SPAN && up * ntp <= RS_LDS_TAPS;
}
template <typename S>
int launch_rate_in(const S* in, long in_stride, float* out, long out_stride, float* rstate, long rs_stride, int N, int nhops,
                   int hin, int up, int down, int ntp, const float* taps, hipStream_t s) {
    if (!rate_geometry_ok(hin, 256, up, down, ntp)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL((k_rate_in<S>), dim3(N), dim3(RS_THREADS), 0, s, in, in_stride, out, out_stride, rstate, rs_stride, nhops,
                       hin, up, down, ntp, taps);
    GT_LAUNCH_CHECK();
    return 0;
}
template <typename S>
int launch_rate_out(const float* in, long in_stride, S* out, long out_stride, float* rstate, long rs_stride, int N, int nhops,
                    int hout, int up, int down, int ntp, const float* taps, hipStream_t s) {
    if (!rate_geometry_ok(256, hout, up, down, ntp)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL((k_rate_out<S>), dim3(N), dim3(RS_THREADS), 0, s, in, in_stride, out, out_stride, rstate, rs_stride, nhops,
                       hout, up, down, ntp, taps);
    GT_LAUNCH_CHECK();
    return 0;
}
template int launch_rate_in<float>(const float*, long, float*, long, float*, long, int, int, int, int, int, int, const float*, hipStream_t);
template int launch_rate_in<short>(const short*, long, float*, long, float*, long, int, int, int, int, int, int, const float*, hipStream_t);
template int launch_rate_out<float>(const float*, long, float*, long, float*, long, int, int, int, int, int, int, const float*, hipStream_t);
template int launch_rate_out<short>(const float*, long, short*, long, float*, long, int, int, int, int, int, int, const float*, hipStream_t);

// ===================================================================== high band (gtcrn_rate_stream_step_hb, gtcrn_resample_hb)
// The band above 8 kHz of a 24 / 32 / 48 kHz stream goes AROUND the model (include/gtcrn_micro_hip.h, "high band"): with
// g the stream's high-band gain, a the 16 kHz hand-off of k_rate_in and w what the wave step emitted for it one hop late,
//     s[k] = w[k] - g a[k - 256]       out[n] = outbound stage(s)[n] + g x[n - lat]       lat = H + 2 D
// every product and sum ONE fp32 rounding (__fmul_rn / __fsub_rn / __fadd_rn: no contraction into an fma).  Both stages are
// linear phase with whole delays that sum to lat, so the stage applied to -g a removes from g x[n - lat] exactly the band
// the model path carries.  k_rate_out_hb is k_rate_out with s staged instead of w -- the same rs_dot on the same layout --
// and the dry term added at the store.  Per-stream state row (floats): [the last 256 samples of a | the last lat input
// samples], zeros after a reset; the outbound history of d_rstate holds s.
// One workgroup per stream.  Every word of the three state rows is read before a barrier and written after it: the delay
// line sits in LDS for the whole call (with one hop per call H < lat: part of it survives and moves), the a block and the
// history are read while hop 0 is staged and written after the last hop's outputs.  x is read while other threads write
// out: the rows must not overlap (gtcrn_rate_stream_step_hb checks).
template <typename S>
__global__ __launch_bounds__(RS_THREADS) void k_rate_out_hb(const float* __restrict__ wet, const float* __restrict__ dry,
                                                            long hand_stride, const S* __restrict__ in, long in_stride,
                                                            S* __restrict__ out, long out_stride, float* __restrict__ rstate,
                                                            long rs_stride, float* __restrict__ hbstate,
                                                            const float* __restrict__ hb_gain, int nhops, int hout, int lat,
                                                            int up, int down, int ntp, const float* __restrict__ taps) {
    __shared__ __attribute__((aligned(16))) float s_x[RATE_SPAN];
    __shared__ __attribute__((aligned(16))) float s_t[RS_LDS_TAPS];
    __shared__ float s_dl[HB_DELAY];
    const int tid = threadIdx.x;
    const long n = blockIdx.x;
    const float g = hb_gain[n];
    const float* w = wet + n * hand_stride;
    const float* a = dry + n * hand_stride;
    const S* x = in + n * in_stride;
    S* o = out + n * out_stride;
    float* hist = rstate + n * rs_stride;
    float* sa = hbstate + n * (256 + lat);
    float* dl = sa + 256;
    const float* tp = rs_stage_taps(taps, up * ntp, s_t, tid, RS_THREADS);      // (never nullptr: launch_rate_out_hb checks)
    for (int i = tid; i < lat; i += RS_THREADS) s_dl[i] = dl[i];
    for (int h = 0; h < nhops; ++h) {
        for (int i = tid; i < ntp + 256; i += RS_THREADS) {
            const long k = (long)h * 256 + i - ntp;
            float v;
            if (k >= 0) v = __fsub_rn(w[k], __fmul_rn(g, k >= 256 ? a[k - 256] : sa[k]));
            else v = hist[ntp + k];
            s_x[i] = v;
        }
        __syncthreads();
        for (int m = tid; m < hout; m += RS_THREADS) {
            const int num = m * down, ih = num / up, k0 = num - ih * up;
            const long j = (long)h * hout + m;
            const float xd = j >= lat ? wave_ld<S>(x + (j - lat)) : s_dl[j];
            wave_st<S>(o + j, __fadd_rn(rs_dot(tp + k0 * ntp, ntp, s_x + ntp + ih), __fmul_rn(g, xd)));
        }
        if (h == nhops - 1)
            for (int i = tid; i < ntp; i += RS_THREADS) hist[i] = s_x[256 + i];
        __syncthreads();
    }
    for (int i = tid; i < 256; i += RS_THREADS) sa[i] = a[(long)(nhops - 1) * 256 + i];
    for (int i = tid; i < lat; i += RS_THREADS) {
        const long p = (long)nhops * hout - lat + i;
        dl[i] = p >= 0 ? wave_ld<S>(x + p) : s_dl[(long)nhops * hout + i];
    }
}

// Batch form, 16 kHz -> fs: k_resample with fl(wet - fl(g dry)) staged instead of the input row and fl(g x[j]) added at the
// store for j < the row's length at fs (outputs of a length-rounding tail past it get no dry term).  Rows have their own
// lengths: lens (device; nullptr: all L) at 16 kHz, xlens (device; nullptr: all Lx) at fs.
__global__ __launch_bounds__(RS_THREADS) void k_resample_hb(const float* __restrict__ wet, long wet_stride,
                                                            const float* __restrict__ dry, long dry_stride,
                                                            const int* __restrict__ lens, long L, const float* __restrict__ xin,
                                                            long x_stride, const int* __restrict__ xlens, long Lx,
                                                            const float* __restrict__ hb_gain, float* __restrict__ out,
                                                            long out_stride, int tiles, int up, int down, int half, int ntp,
                                                            const float* __restrict__ taps, int vec) {
    __shared__ __attribute__((aligned(16))) float s_x[RS_SPAN];
    __shared__ __attribute__((aligned(16))) float s_t[RS_LDS_TAPS];
    const int tid = threadIdx.x;
    const int row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
    long len = lens ? (long)lens[row] : L;
    len = len < 0 ? 0 : (len > L ? L : len);
    long xlen = xlens ? (long)xlens[row] : Lx;
    xlen = xlen < 0 ? 0 : (xlen > Lx ? Lx : xlen);
    const long nout = (len * up + down - 1) / down;
    const long j0 = (long)tile * RS_TILE;
    if (j0 >= nout) return;                                         // (workgroup uniform)
    const long j1 = j0 + RS_TILE < nout ? j0 + RS_TILE : nout;
    const float g = hb_gain[row];
    const float* tp = rs_stage_taps(taps, up * ntp, s_t, tid, RS_THREADS);      // (never nullptr: launch_resample_hb checks)
    const long lo = (j0 * down + half) / up - (ntp - 1), hi = ((j1 - 1) * down + half) / up;
    const long a0 = lo - (((lo % 4) + 4) % 4);                     // the span starts on a 16-byte boundary of the rows
    const int nv = (int)((hi - a0) / 4) + 1;                       // nv * 4 <= RS_SPAN: launch_resample_hb checks the worst tile
    const float* w = wet + (long)row * wet_stride;
    const float* d = dry + (long)row * dry_stride;
    for (int v = tid; v < nv; v += RS_THREADS) {
        const long i = a0 + (long)v * 4;
        f32x4 f;
        if (vec && i >= 0 && i + 4 <= len) {
            const f32x4 qw = *reinterpret_cast<const f32x4*>(w + i), qd = *reinterpret_cast<const f32x4*>(d + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) f[e] = __fsub_rn(qw[e], __fmul_rn(g, qd[e]));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) f[e] = (i + e >= 0 && i + e < len) ? __fsub_rn(w[i + e], __fmul_rn(g, d[i + e])) : 0.f;
        }
        st4(s_x + v * 4, f);
    }
    __syncthreads();
    const float* x = xin + (long)row * x_stride;
    float* o = out + (long)row * out_stride;
    for (long j = j0 + tid; j < j1; j += RS_THREADS) {
        const long num = j * down + half, ih = num / up;
        const int k0 = (int)(num - ih * up);
        const float y = rs_dot(tp + k0 * ntp, ntp, s_x + (ih - a0));
        o[j] = j < xlen ? __fadd_rn(y, __fmul_rn(g, x[j])) : y;
    }
}

template <typename S>
int launch_rate_out_hb(const float* wet, const float* dry, long hand_stride, const S* in, long in_stride, S* out, long out_stride,
                       float* rstate, long rs_stride, float* hbstate, const float* hb_gain, int N, int nhops, int hout, int lat,
                       int up, int down, int ntp, const float* taps, hipStream_t s) {
    if (!rate_geometry_ok(256, hout, up, down, ntp) || lat < 1 || lat > HB_DELAY || (lat & 3)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL((k_rate_out_hb<S>), dim3(N), dim3(RS_THREADS), 0, s, wet, dry, hand_stride, in, in_stride, out, out_stride,
                       rstate, rs_stride, hbstate, hb_gain, nhops, hout, lat, up, down, ntp, taps);
    GT_LAUNCH_CHECK();
    return 0;
}
template int launch_rate_out_hb<float>(const float*, const float*, long, const float*, long, float*, long, float*, long, float*,
                                       const float*, int, int, int, int, int, int, int, const float*, hipStream_t);
template int launch_rate_out_hb<short>(const float*, const float*, long, const short*, long, short*, long, float*, long, float*,
                                       const float*, int, int, int, int, int, int, int, const float*, hipStream_t);

int launch_resample_hb(const float* wet, long wet_stride, const float* dry, long dry_stride, const int* lens, long L,
                       const float* x, long x_stride, const int* xlens, long Lx, const float* hb_gain, float* out,
                       long out_stride, int B, int up, int down, int half, int ntp, const float* taps, hipStream_t s) {
    if (resample_tile_span(up, down, ntp) > RS_SPAN || (ntp & 3) || up * ntp > RS_LDS_TAPS ||
        (reinterpret_cast<uintptr_t>(taps) & 15))
        return (int)hipErrorInvalidValue;
    const long nout = (L * up + down - 1) / down;
    const long tiles = (nout + RS_TILE - 1) / RS_TILE;
    if (tiles < 1 || tiles * B > 0x7fffffffL) return (int)hipErrorInvalidValue;
    const int vec = !((reinterpret_cast<uintptr_t>(wet) | reinterpret_cast<uintptr_t>(dry)) & 15) && wet_stride % 4 == 0 &&
                    dry_stride % 4 == 0;
    hipLaunchKernelGGL(k_resample_hb, dim3((unsigned)(tiles * B)), dim3(RS_THREADS), 0, s, wet, wet_stride, dry, dry_stride, lens,
                       L, x, x_stride, xlens, Lx, hb_gain, out, out_stride, (int)tiles, up, down, half, ntp, taps, vec);
    GT_LAUNCH_CHECK();
    return 0;
}

// ===================================================================== packet-sized live streaming (gtcrn_packet_stream_*)
// A caller's packet of n samples at fs (n16 = n 16000 / fs samples at 16 kHz, a whole number) in, n enhanced samples out,
// around the UNCHANGED wave step: k_packet_in cuts the group's 16 kHz sample sequence into 256-sample hops, k_packet_out
// cuts the hops the wave step emits back into packets.  The group's phase phi = (16 kHz samples taken so far) mod 256
// lives on the host and is the same for every stream, and so are both FIFO levels: the inbound FIFO holds phi samples
// between calls, the outbound one lvl = 256 - gcd(n16, 256) - phi.  A call steps h = (phi + n16) div 256 hops (host
// arithmetic, possibly 0).  Neither level is stored: a reset is a memset, and a stream reset at phase z thereby holds z
// zeros inbound and 256 - g - z zeros outbound, which is its pre-roll.  Per-stream state row (floats):
// [inbound FIFO PK_FIFO | outbound FIFO PK_FIFO | inbound stage history ntp_in | outbound stage history ntp_out].
//
// The resampling stages (fs != 16000) are the causal forms of rate_hops on the same values through the same rs_dot: output
// m of a packet reads the packet's inputs up to (m down) div up (n up == n16 down: every packet starts at filter phase 0)
// and back ntp - 1 samples, into the stream's history.  The inbound stage walks the packet in rounds of PK_TILE outputs
// whose input span it stages in LDS (a packet at 48 kHz may hold 12 288 samples); the outbound stage reads the popped 16 kHz
// packet where it already sits in LDS, its history in front of it.  Phase tables above RS_LDS_TAPS floats (44.1 / 22.05
// kHz) are read from global memory, as k_resample does.
// One workgroup per stream.  Every global word of the state row is read into LDS before the barrier and written after it
// by the thread that owns its index; nothing is read back.
// Where sample i of a call's row (hop i >> 8, place i & 255) sits in a hand-off buffer.  Contiguous: row-major, `stride`
// floats apart.  Indexed: round-major, block r is M rows of 256 floats and hop r of a row is row pos[r M + row] of it.
// (RS_THREADS == 256: a thread's hop index i >> 8 is workgroup uniform in every pass of a loop over i.)
template <bool IDX>
struct PkHand {
    long stride;          // contiguous
    const int* pos;       // indexed
    int M;
    __device__ __forceinline__ long at(long row, int i) const {
        if constexpr (IDX) return ((long)(i >> 8) * M + pos[(long)(i >> 8) * M + row]) * 256 + (i & 255);
        else return row * stride + i;
    }
};

// The inbound stage and FIFO of one stream: ONE statement for k_packet_in and k_packet_in_slots, which resolve srow (the
// stream's row of pstate: the call's row, or its slot) and phi / h (the group's, or the row's from the plan record).
template <bool IDX, typename S>
__device__ __forceinline__ void packet_in_body(const S* __restrict__ in, long in_stride, int n, float* __restrict__ hand,
                                               PkHand<IDX> hd, float* __restrict__ pstate, long ps_stride, long srow, int phi,
                                               int n16, int h, int up, int down, int ntp, const float* __restrict__ taps) {
    __shared__ __attribute__((aligned(16))) float s_a[PK_SEQ];       // the FIFO's phi samples ++ this packet at 16 kHz
    __shared__ __attribute__((aligned(16))) float s_x[PK_SPAN];
    __shared__ __attribute__((aligned(16))) float s_t[RS_LDS_TAPS];
    const int tid = threadIdx.x;
    const long row = blockIdx.x;
    const S* x = in + row * in_stride;
    float* ps = pstate + srow * ps_stride;
    for (int i = tid; i < phi; i += RS_THREADS) s_a[i] = ps[i];
    if (ntp == 0) {                                                  // 16 kHz: the packet as it is
        for (int m = tid; m < n16; m += RS_THREADS) s_a[phi + m] = wave_ld<S>(x + m);
        __syncthreads();
    } else {
        float* hist = ps + 2 * PK_FIFO;
        const float* tp = rs_stage_taps(taps, up * ntp, s_t, tid, RS_THREADS);
        for (int m0 = 0; m0 < n16; m0 += PK_TILE) {
            const int m1 = m0 + PK_TILE < n16 ? m0 + PK_TILE : n16;
            const int lo = (m0 * down) / up - (ntp - 1), cnt = ((m1 - 1) * down) / up - lo + 1;   // <= PK_SPAN (launch check)
            for (int i = tid; i < cnt; i += RS_THREADS) {
                const int g = lo + i;                                // >= 1 - ntp; < n
                s_x[i] = g >= 0 ? wave_ld<S>(x + g) : hist[ntp + g];
            }
            __syncthreads();
            for (int m = m0 + tid; m < m1; m += RS_THREADS) {
                const int num = m * down, ih = num / up, k0 = num - ih * up;
                const float* xs = s_x + (ih - lo);
                s_a[phi + m] = tp ? rs_dot(tp + k0 * ntp, ntp, xs) : rs_dot(taps + (long)k0 * ntp, ntp, xs);
            }
            __syncthreads();
        }
        for (int i = tid; i < ntp; i += RS_THREADS) hist[i] = wave_ld<S>(x + n - ntp + i);        // (ntp <= n)
    }
    const int whole = 256 * h, rem = phi + n16 - whole;              // rem < 256: the next call's phi
    for (int i = tid; i < whole; i += RS_THREADS) hand[hd.at(row, i)] = s_a[i];
    for (int i = tid; i < rem; i += RS_THREADS) ps[i] = s_a[whole + i];
}

// What the high-band kernels take beyond the plain outbound ones (an empty record in the plain kernels, never read).
template <typename S>
struct PkHbArgs {
    const float* hand_a = nullptr;    // the inbound hand-off of the same call, read only
    const S* in = nullptr;            // the call's input rows
    long in_stride = 0;
    float* hbstate = nullptr;
    long hb_stride = 0;
    const float* hb_gain = nullptr;
    int l16 = 0, lat = 0, phi = 0;    // phi: the phase BEFORE this call's inbound stage
};

// The outbound FIFO and stage of one stream: ONE statement for k_packet_out, k_packet_out_slots and (HB) their high-band
// forms; the kernels resolve srow, lvl and h as the inbound ones do.
// HB carries the band above 8 kHz around the model.  With gam = hb_gain[srow], A the stream's inbound 16 kHz sequence and P
// what the outbound FIFO pops (both counted from the stream's reset), l16 = 512 - g and lat the form's latency at fs:
//     s[t] = fl(P[t] - fl(gam A[t - l16]))   staged in the place of the n16 popped samples (the remainder that returns to the
//                                            FIFO stays raw P; the outbound history then holds s)
//     out[m] = fl(stage(s)[m] + fl(gam x[m - lat]))
// High-band state row (floats, hb_stride apart): [the last l16 samples of A | the last lat input samples], zeros after a
// reset.  This call's n16 new samples of A are where k_packet_in left them: index phi + k of "old inbound FIFO ++ packet" lies
// in hop (phi + k) >> 8 of the inbound hand-off while below 256 h, else in the inbound FIFO of the packet state (neither is
// written here; the wave step writes the other hand-off).  The HB form assumes a stage (ntp > 0) whose table fits LDS: the
// launcher checks both.
// Every word of the state rows is read into LDS before the barrier and written after it by the thread that owns its index:
// with n < lat most of the delay line survives a call and moves.
template <bool IDX, bool HB, typename S>
__device__ __forceinline__ void packet_out_body(const float* __restrict__ hand, PkHand<IDX> hd, S* __restrict__ out,
                                                long out_stride, int n, float* __restrict__ pstate, long ps_stride, int hist_off,
                                                long srow, int lvl, int n16, int h, int up, int down, int ntp,
                                                const float* __restrict__ taps, const PkHbArgs<S> hb) {
    __shared__ __attribute__((aligned(16))) float s_q[PK_HIST + PK_SEQ];   // [stage history | the FIFO's lvl samples ++ 256 h new]
    __shared__ __attribute__((aligned(16))) float s_t[RS_LDS_TAPS];
    [[maybe_unused]] __shared__ float s_sa[HB ? PKHB_A : 1];           // the last l16 samples of A
    [[maybe_unused]] __shared__ float s_dl[HB ? PKHB_DELAY : 1];       // the last lat input samples
    const int tid = threadIdx.x;
    const long row = blockIdx.x;
    float* ps = pstate + srow * ps_stride;
    float* fo = ps + PK_FIFO;
    float* hist = ps + hist_off;
    float* q = s_q + PK_HIST;
    const int whole = 256 * h;
    [[maybe_unused]] const float gam = HB ? hb.hb_gain[srow] : 0.f;
    [[maybe_unused]] float* const sa = hb.hbstate + srow * hb.hb_stride;
    [[maybe_unused]] float* const dl = sa + hb.l16;
    [[maybe_unused]] const S* const x = hb.in + row * hb.in_stride;
    // new sample k < n16 of A (this call's)
    [[maybe_unused]] const auto new_a = [&](int k) -> float {
        const int i = hb.phi + k;
        return i >= whole ? ps[i - whole] : hb.hand_a[hd.at(row, i)];
    };
    // what is staged for popped sample m of this call: P[m], less gam A[t - l16] (the state's, then this call's own) in HB
    const auto staged = [&](int m, float p) -> float {
        if constexpr (HB) {
            if (m < n16) return __fsub_rn(p, __fmul_rn(gam, m < hb.l16 ? sa[m] : new_a(m - hb.l16)));
        }
        return p;
    };
    for (int i = tid; i < lvl; i += RS_THREADS) q[i] = staged(i, fo[i]);
    for (int i = tid; i < whole; i += RS_THREADS) q[lvl + i] = staged(lvl + i, hand[hd.at(row, i)]);
    for (int i = tid; i < ntp; i += RS_THREADS) q[i - ntp] = hist[i];
    if constexpr (HB) {
        for (int i = tid; i < hb.l16; i += RS_THREADS) s_sa[i] = sa[i];
        for (int i = tid; i < hb.lat; i += RS_THREADS) s_dl[i] = dl[i];
    }
    const float* tp = HB || ntp ? rs_stage_taps(taps, up * ntp, s_t, tid, RS_THREADS) : nullptr;   // (HB: never nullptr)
    __syncthreads();
    S* o = out + row * out_stride;
    if (!HB && ntp == 0) {
        for (int m = tid; m < n; m += RS_THREADS) wave_st<S>(o + m, q[m]);
    } else {
        for (int m = tid; m < n; m += RS_THREADS) {
            const int num = m * down, ih = num / up, k0 = num - ih * up;       // ih < n16
            const float y = HB || tp ? rs_dot(tp + k0 * ntp, ntp, q + ih) : rs_dot(taps + (long)k0 * ntp, ntp, q + ih);
            if constexpr (HB) {
                const float xd = m >= hb.lat ? wave_ld<S>(x + (m - hb.lat)) : s_dl[m];
                wave_st<S>(o + m, __fadd_rn(y, __fmul_rn(gam, xd)));
            } else {
                wave_st<S>(o + m, y);
            }
        }
        for (int i = tid; i < ntp; i += RS_THREADS) hist[i] = q[n16 - ntp + i];
    }
    const int rem = lvl + whole - n16;                               // < 256: the next call's lvl
    for (int i = tid; i < rem; i += RS_THREADS) fo[i] = q[n16 + i];
    if constexpr (HB) {
        // both delay lines advance: the last l16 of (A's line ++ n16 new), the last lat of (x's line ++ the packet)
        for (int i = tid; i < hb.l16; i += RS_THREADS) sa[i] = n16 + i < hb.l16 ? s_sa[n16 + i] : new_a(n16 + i - hb.l16);
        for (int i = tid; i < hb.lat; i += RS_THREADS) dl[i] = n + i < hb.lat ? s_dl[n + i] : wave_ld<S>(x + (n + i - hb.lat));
    }
}

template <typename S>
__global__ __launch_bounds__(RS_THREADS) void k_packet_in(const S* __restrict__ in, long in_stride, int n, float* __restrict__ hand,
                                                          long hand_stride, float* __restrict__ pstate, long ps_stride, int phi,
                                                          int n16, int h, int up, int down, int ntp,
                                                          const float* __restrict__ taps) {
    packet_in_body<false, S>(in, in_stride, n, hand, {hand_stride, nullptr, 0}, pstate, ps_stride, blockIdx.x, phi, n16, h, up,
                             down, ntp, taps);
}

template <typename S>
__global__ __launch_bounds__(RS_THREADS) void k_packet_out(const float* __restrict__ hand, long hand_stride, S* __restrict__ out,
                                                           long out_stride, int n, float* __restrict__ pstate, long ps_stride,
                                                           int hist_off, int lvl, int n16, int h, int up, int down, int ntp,
                                                           const float* __restrict__ taps) {
    packet_out_body<false, false, S>(hand, {hand_stride, nullptr, 0}, out, out_stride, n, pstate, ps_stride, hist_off, blockIdx.x,
                                     lvl, n16, h, up, down, ntp, taps, {});
}

// ---- packet stream slots (gtcrn_packet_stream_*_slots): the packet form for the resident streams a call names.  The phase
// is one device word per slot, so every stream runs the schedule of a one-stream group created at phase 0 whatever the
// others do.  A call is plan -> k_packet_in_slots -> hmax rounds of the indexed single-launch wave step -> k_packet_out_slots,
// whatever the phases: round r steps the rows that have more than r hops ready, named by the table the plan wrote.
//
// k_packet_plan, ONE workgroup: for row i < count (clamped) it reads slot = slots[i] and phi = phase[slot], h_i = (phi + n16)
// div 256, and writes the row's record (phi_rec[i] = phi, pos[r M + i] = the row's place in round r's table or -1), the
// tables tab[r M + j] = slot IN ROW ORDER (an exclusive scan of "h_i > r" over the rows: wave ballots, the waves' counts
// through LDS, a running base per round), the rounds' counts, and phase[slot] = (phi + n16) mod 256.  The later kernels
// read the record, never `phase`.  A phase word the schedule cannot reach (a slot that was never reset) is masked into
// 0..255 and, if it would still give more than hmax hops, read as 0: no later index depends on the caller's memory.  PLAN_THREADS rows per pass, three barriers a pass.
constexpr int PK_HMAX = (255 + PK_MAX16) / 256;  // the most rounds any packet takes (16)
constexpr int PLAN_THREADS = 1024, PLAN_WAVES = PLAN_THREADS / 64;
__global__ __launch_bounds__(PLAN_THREADS) void k_packet_plan(const int* __restrict__ slots, const int* __restrict__ count,
                                                              int max_active, int* __restrict__ phase, int n16, int hmax, int M,
                                                              int* __restrict__ tab, int* __restrict__ pos,
                                                              int* __restrict__ phi_rec, int* __restrict__ cnts) {
    __shared__ int s_wc[PK_HMAX][PLAN_WAVES];
    __shared__ int s_base[PK_HMAX];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int N = slot_count(count, max_active);
    if (tid < PK_HMAX) s_base[tid] = 0;
    __syncthreads();
    for (int i0 = 0; i0 < N; i0 += PLAN_THREADS) {                   // (workgroup uniform)
        const int i = i0 + tid;
        const bool live = i < N;
        int slot = 0, h = 0;
        if (live) {
            slot = slots[i];
            int phi = phase[slot] & 255;
            if (((phi + n16) >> 8) > hmax) phi = 0;                  // (no phase the schedule reaches: see above)
            h = (phi + n16) >> 8;
            phase[slot] = (phi + n16) & 255;
            phi_rec[i] = phi;
        }
        for (int r = 0; r < hmax; ++r) {
            const unsigned long long b = __ballot(h > r);
            if (lane == 0) s_wc[r][wv] = __popcll(b);
        }
        __syncthreads();
        for (int r = 0; r < hmax; ++r) {
            const unsigned long long b = __ballot(h > r);
            int j = s_base[r] + __popcll(b & ((1ull << lane) - 1ull));
            for (int w = 0; w < wv; ++w) j += s_wc[r][w];
            if (live) {
                pos[(long)r * M + i] = h > r ? j : -1;
                if (h > r) tab[(long)r * M + j] = slot;
            }
        }
        __syncthreads();
        if (tid < hmax) {
            int t = s_base[tid];
            for (int w = 0; w < PLAN_WAVES; ++w) t += s_wc[tid][w];
            s_base[tid] = t;
        }
        __syncthreads();
    }
    if (tid < hmax) cnts[tid] = s_base[tid];
}

// k_packet_in_slots / k_packet_out_slots: packet_in_body / packet_out_body with the state row taken at the slot, phi / h /
// lvl per row from the plan record, and the hand-off addressed through PkHand<true> (round-major: hop r of a row is row
// pos[r M + row] of round r's block of M rows of 256 floats).  A workgroup at or beyond the count returns before its first
// barrier and state access.
template <typename S>
__global__ __launch_bounds__(RS_THREADS) void k_packet_in_slots(const S* __restrict__ in, long in_stride, int n,
                                                                float* __restrict__ hand, int M, float* __restrict__ pstate,
                                                                long ps_stride, const int* __restrict__ slots,
                                                                const int* __restrict__ count, int max_active,
                                                                const int* __restrict__ phi_rec, const int* __restrict__ pos,
                                                                int n16, int up, int down, int ntp,
                                                                const float* __restrict__ taps) {
    if ((int)blockIdx.x >= slot_count(count, max_active)) return;
    const int phi = phi_rec[blockIdx.x];
    packet_in_body<true, S>(in, in_stride, n, hand, {0, pos, M}, pstate, ps_stride, slots[blockIdx.x], phi, n16, (phi + n16) >> 8,
                            up, down, ntp, taps);
}

template <typename S>
__global__ __launch_bounds__(RS_THREADS) void k_packet_out_slots(const float* __restrict__ hand, int M, S* __restrict__ out,
                                                                 long out_stride, int n, float* __restrict__ pstate,
                                                                 long ps_stride, int hist_off, const int* __restrict__ slots,
                                                                 const int* __restrict__ count, int max_active,
                                                                 const int* __restrict__ phi_rec, const int* __restrict__ pos,
                                                                 int g, int n16, int up, int down, int ntp,
                                                                 const float* __restrict__ taps) {
    if ((int)blockIdx.x >= slot_count(count, max_active)) return;
    const int phi = phi_rec[blockIdx.x];
    packet_out_body<true, false, S>(hand, {0, pos, M}, out, out_stride, n, pstate, ps_stride, hist_off, slots[blockIdx.x],
                                    256 - g - phi, n16, (phi + n16) >> 8, up, down, ntp, taps, {});
}

// zeroes the packet state rows and the phase words of the listed slots (with k_reset_slots: gtcrn_packet_stream_reset_slots)
__global__ __launch_bounds__(RS_THREADS) void k_packet_reset_slots(float* __restrict__ pstate, long ps_stride,
                                                                   int* __restrict__ phase, const int* __restrict__ slots,
                                                                   const int* __restrict__ count, int max_active) {
    if ((int)blockIdx.x >= slot_count(count, max_active)) return;
    const long slot = slots[blockIdx.x];
    float* ps = pstate + slot * ps_stride;
    for (int i = threadIdx.x; i < ps_stride; i += RS_THREADS) ps[i] = 0.f;
    if (threadIdx.x == 0) phase[slot] = 0;
}

// ---- high band on the packet forms (gtcrn_packet_stream_step_hb, _step_slots_hb): k_packet_out / k_packet_out_slots with
// the band above 8 kHz carried around the model (packet_out_body<IDX, true> states the arithmetic and the state row).  They take
// BOTH hand-offs (hand_a: what the inbound kernel produced, read only), the call's input rows, the old inbound phase and
// the high-band state and gains; the gain and the state row are the stream's (by row, or by slot).
template <typename S>
__global__ __launch_bounds__(RS_THREADS) void k_packet_out_hb(const float* __restrict__ hand, const float* __restrict__ hand_a,
                                                              long hand_stride, const S* __restrict__ in, long in_stride,
                                                              S* __restrict__ out, long out_stride, int n,
                                                              float* __restrict__ pstate, long ps_stride, int hist_off,
                                                              float* __restrict__ hbstate, long hb_stride,
                                                              const float* __restrict__ hb_gain, int l16, int lat, int phi,
                                                              int lvl, int n16, int h, int up, int down, int ntp,
                                                              const float* __restrict__ taps) {
    packet_out_body<false, true, S>(hand, {hand_stride, nullptr, 0}, out, out_stride, n, pstate, ps_stride, hist_off, blockIdx.x,
                                    lvl, n16, h, up, down, ntp, taps,
                                    {hand_a, in, in_stride, hbstate, hb_stride, hb_gain, l16, lat, phi});
}

template <typename S>
__global__ __launch_bounds__(RS_THREADS) void k_packet_out_slots_hb(const float* __restrict__ hand, const float* __restrict__ hand_a,
                                                                    int M, const S* __restrict__ in, long in_stride,
                                                                    S* __restrict__ out, long out_stride, int n,
                                                                    float* __restrict__ pstate, long ps_stride, int hist_off,
                                                                    float* __restrict__ hbstate, long hb_stride,
                                                                    const float* __restrict__ hb_gain, int l16, int lat,
                                                                    const int* __restrict__ slots, const int* __restrict__ count,
                                                                    int max_active, const int* __restrict__ phi_rec,
                                                                    const int* __restrict__ pos, int g, int n16, int up,
                                                                    int down, int ntp, const float* __restrict__ taps) {
    if ((int)blockIdx.x >= slot_count(count, max_active)) return;
    const int phi = phi_rec[blockIdx.x];
    packet_out_body<true, true, S>(hand, {0, pos, M}, out, out_stride, n, pstate, ps_stride, hist_off, slots[blockIdx.x],
                                   256 - g - phi, n16, (phi + n16) >> 8, up, down, ntp, taps,
                                   {hand_a, in, in_stride, hbstate, hb_stride, hb_gain, l16, lat, phi});
}

// zeroes the high-band rows of the listed slots (gtcrn_packet_stream_hb_reset_slots)
__global__ __launch_bounds__(RS_THREADS) void k_packet_hb_reset_slots(float* __restrict__ hbstate, long hb_stride,
                                                                      const int* __restrict__ slots,
                                                                      const int* __restrict__ count, int max_active) {
    if ((int)blockIdx.x >= slot_count(count, max_active)) return;
    float* hb = hbstate + (long)slots[blockIdx.x] * hb_stride;
    for (int i = threadIdx.x; i < hb_stride; i += RS_THREADS) hb[i] = 0.f;
}

static bool packet_stage_ok(int n_in, int n_out, int up, int down, int ntp, const float* taps) {
    if (ntp == 0) return n_in == n_out;
    return taps && !(reinterpret_cast<uintptr_t>(taps) & 15) && up >= 1 && down >= 1 && (long)n_in * up == (long)n_out * down &&
           !(ntp & 3) && ntp <= n_in;
}
// what both step launchers check: the packet, the rows of the form, and the phase the contiguous form is given
static bool packet_rows_ok(const PkPacket& pk, const PkRows& rw) {
    if (pk.n16 < 1 || pk.n16 > PK_MAX16) return false;
    if (rw.rows.slots) return rw.N >= 1 && rw.N <= rw.M;
    return rw.phi >= 0 && rw.phi < 256 && rw.hand_stride >= 256L * ((rw.phi + pk.n16) / 256);
}
template <typename S>
int launch_packet_in(const S* in, long in_stride, float* hand, PkPacket pk, PkState st, PkRows rw, PkStage sg, hipStream_t s) {
    if (!packet_rows_ok(pk, rw) || st.ps_stride < 2 * PK_FIFO + sg.ntp ||
        !packet_stage_ok(pk.n, pk.n16, sg.up, sg.down, sg.ntp, sg.taps) ||
        (sg.ntp && ((PK_TILE - 1) * sg.down) / sg.up + sg.ntp + 1 > PK_SPAN))
        return (int)hipErrorInvalidValue;
    if (rw.rows.slots) {
        hipLaunchKernelGGL((k_packet_in_slots<S>), dim3(rw.N), dim3(RS_THREADS), 0, s, in, in_stride, pk.n, hand, rw.M, st.pstate,
                           st.ps_stride, rw.rows.slots, rw.rows.cnt, rw.N, rw.phi_rec, rw.pos, pk.n16, sg.up, sg.down, sg.ntp,
                           sg.taps);
    } else {
        hipLaunchKernelGGL((k_packet_in<S>), dim3(rw.N), dim3(RS_THREADS), 0, s, in, in_stride, pk.n, hand, rw.hand_stride,
                           st.pstate, st.ps_stride, rw.phi, pk.n16, (rw.phi + pk.n16) / 256, sg.up, sg.down, sg.ntp, sg.taps);
    }
    GT_LAUNCH_CHECK();
    return 0;
}
template <typename S>
int launch_packet_out(const float* hand, const S* in, long in_stride, S* out, long out_stride, PkPacket pk, PkState st,
                      PkRows rw, PkStage sg, const PkHighBand* hb, hipStream_t s) {
    constexpr bool kHb = std::is_same<S, float>::value || std::is_same<S, short>::value;   // (no G.711 high-band kernel exists)
    // contiguous: the hops and both FIFO levels follow from the group's phase, a multiple of g on every schedule
    const int h = (rw.phi + pk.n16) / 256, lvl = 256 - pk.g - rw.phi, rem = lvl + 256 * h - pk.n16;
    if (!packet_rows_ok(pk, rw) || pk.g < 1 || pk.g > 256 || 256 % pk.g || pk.n16 % pk.g || st.hist_off < 2 * PK_FIFO ||
        st.ps_stride < st.hist_off + sg.ntp || sg.ntp > PK_HIST || !packet_stage_ok(pk.n16, pk.n, sg.up, sg.down, sg.ntp, sg.taps))
        return (int)hipErrorInvalidValue;
    if (!rw.rows.slots && (lvl < 0 || rem < 0)) return (int)hipErrorInvalidValue;
    // the high band: the stage exists (ntp > 0) and its table sits in LDS
    if (hb && (!kHb || !hb->hand_a || !in || !hb->hbstate || !hb->gain || hb->l16 != 512 - pk.g || hb->l16 < 256 ||
               hb->l16 > PKHB_A || hb->lat < 1 || hb->lat > PKHB_DELAY || hb->hb_stride < hb->l16 + hb->lat || sg.ntp <= 0 ||
               sg.up * sg.ntp > RS_LDS_TAPS))
        return (int)hipErrorInvalidValue;
    const dim3 grid(rw.N), block(RS_THREADS);
    if (hb) {
        if constexpr (kHb) {
            if (rw.rows.slots) {
                hipLaunchKernelGGL((k_packet_out_slots_hb<S>), grid, block, 0, s, hand, hb->hand_a, rw.M, in, in_stride, out,
                                   out_stride, pk.n, st.pstate, st.ps_stride, st.hist_off, hb->hbstate, hb->hb_stride, hb->gain,
                                   hb->l16, hb->lat, rw.rows.slots, rw.rows.cnt, rw.N, rw.phi_rec, rw.pos, pk.g, pk.n16, sg.up,
                                   sg.down, sg.ntp, sg.taps);
            } else {
                hipLaunchKernelGGL((k_packet_out_hb<S>), grid, block, 0, s, hand, hb->hand_a, rw.hand_stride, in, in_stride, out,
                                   out_stride, pk.n, st.pstate, st.ps_stride, st.hist_off, hb->hbstate, hb->hb_stride, hb->gain,
                                   hb->l16, hb->lat, rw.phi, lvl, pk.n16, h, sg.up, sg.down, sg.ntp, sg.taps);
            }
        }
    } else if (rw.rows.slots) {
        hipLaunchKernelGGL((k_packet_out_slots<S>), grid, block, 0, s, hand, rw.M, out, out_stride, pk.n, st.pstate, st.ps_stride,
                           st.hist_off, rw.rows.slots, rw.rows.cnt, rw.N, rw.phi_rec, rw.pos, pk.g, pk.n16, sg.up, sg.down,
                           sg.ntp, sg.taps);
    } else {
        hipLaunchKernelGGL((k_packet_out<S>), grid, block, 0, s, hand, rw.hand_stride, out, out_stride, pk.n, st.pstate,
                           st.ps_stride, st.hist_off, lvl, pk.n16, h, sg.up, sg.down, sg.ntp, sg.taps);
    }
    GT_LAUNCH_CHECK();
    return 0;
}
template int launch_packet_in<float>(const float*, long, float*, PkPacket, PkState, PkRows, PkStage, hipStream_t);
template int launch_packet_in<short>(const short*, long, float*, PkPacket, PkState, PkRows, PkStage, hipStream_t);
template int launch_packet_in<g711u>(const g711u*, long, float*, PkPacket, PkState, PkRows, PkStage, hipStream_t);
template int launch_packet_in<g711a>(const g711a*, long, float*, PkPacket, PkState, PkRows, PkStage, hipStream_t);
template int launch_packet_out<float>(const float*, const float*, long, float*, long, PkPacket, PkState, PkRows, PkStage, const PkHighBand*, hipStream_t);
template int launch_packet_out<short>(const float*, const short*, long, short*, long, PkPacket, PkState, PkRows, PkStage, const PkHighBand*, hipStream_t);
template int launch_packet_out<g711u>(const float*, const g711u*, long, g711u*, long, PkPacket, PkState, PkRows, PkStage, const PkHighBand*, hipStream_t);
template int launch_packet_out<g711a>(const float*, const g711a*, long, g711a*, long, PkPacket, PkState, PkRows, PkStage, const PkHighBand*, hipStream_t);

// ---- packet stream slots: the launch sequence of a call depends on (fs, n, max_active) alone
int launch_packet_plan(const int* slots, const int* cnt, int max_active, int* phase, int n16, int hmax, int M, int* tab,
                       int* pos, int* phi_rec, int* cnts, hipStream_t s) {
    if (!slots || !phase || max_active < 1 || max_active > M || n16 < 1 || n16 > PK_MAX16 || hmax < n16 / 256 || hmax < 1 ||
        hmax > PK_HMAX)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_packet_plan, dim3(1), dim3(PLAN_THREADS), 0, s, slots, cnt, max_active, phase, n16, hmax, M, tab, pos,
                       phi_rec, cnts);
    GT_LAUNCH_CHECK();
    return 0;
}
int launch_packet_reset_slots(float* pstate, long ps_stride, int* phase, const int* slots, const int* cnt, int max_active,
                              hipStream_t s) {
    if (!pstate || !phase || !slots || max_active < 1 || ps_stride < 2 * PK_FIFO) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_packet_reset_slots, dim3(max_active), dim3(RS_THREADS), 0, s, pstate, ps_stride, phase, slots, cnt,
                       max_active);
    GT_LAUNCH_CHECK();
    return 0;
}
int launch_packet_hb_reset_slots(float* hbstate, long hb_stride, const int* slots, const int* cnt, int max_active,
                                 hipStream_t s) {
    if (!hbstate || !slots || max_active < 1 || hb_stride < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_packet_hb_reset_slots, dim3(max_active), dim3(RS_THREADS), 0, s, hbstate, hb_stride, slots, cnt,
                       max_active);
    GT_LAUNCH_CHECK();
    return 0;
}

}  // namespace gtk
