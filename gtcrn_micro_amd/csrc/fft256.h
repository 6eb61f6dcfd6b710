// fft256.h -- the transform stage of every waveform boundary: device functions only, one definition of each expression.
//
// torch.stft / torch.istft (512 samples, hop 256) as a 256-point complex FFT of the packed frame: table load, window
// product, radix-4 Stockham FFT in LDS (one wave per frame), real-FFT split, inverse merge, (z / 256) * win, overlap-add
// envelope, reflect-padded frame fetch and the PCM16 widening / rounding.  k_stft, k_istft(_mix), k_front, k_wave_analysis,
// k_wave_synthesis, the bulk converters (kernels.hip) and k_score_env (metrics.hip) all call these, so forms that must
// agree bit for bit cannot drift apart: an edit here changes every form alike.  Each file compiles them under its own
// flags (kernels.hip contracts multiply-adds per source expression, which is per expression of THIS file).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gtfft {

// Ordering for LDS data that only the lanes of ONE wave exchange: LDS operations of a wave complete in
// issue order, so it is enough to keep the compiler from reordering across this point.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// 256-point complex FFT of one wave's buffer (ping-pong a -> b ...), DIR = -1 forward, +1 inverse
// (unnormalised).  tw[k] = exp(-2 pi i k / 256).  Result ends in `a` (4 stages).
template <int DIR>
__device__ __forceinline__ void fft256(float2* a, float2* b, const float2* tw, int lane) {
    float2* src = a;
    float2* dst = b;
#pragma unroll
    for (int stage = 0; stage < 4; ++stage) {
        const int Ns = 1 << (2 * stage);
        const int k = lane & (Ns - 1);
        const int tstep = k * (64 / Ns);
        float2 v0 = src[lane], v1 = src[lane + 64], v2 = src[lane + 128], v3 = src[lane + 192];
        if (stage > 0) {
            float2 w1 = tw[tstep], w2 = tw[2 * tstep], w3 = tw[3 * tstep];
            if (DIR > 0) { w1.y = -w1.y; w2.y = -w2.y; w3.y = -w3.y; }
            v1 = cmul(v1, w1); v2 = cmul(v2, w2); v3 = cmul(v3, w3);
        }
        const float2 s0 = make_float2(v0.x + v2.x, v0.y + v2.y), s1 = make_float2(v0.x - v2.x, v0.y - v2.y);
        const float2 s2 = make_float2(v1.x + v3.x, v1.y + v3.y);
        const float2 dd = make_float2(v1.x - v3.x, v1.y - v3.y);
        // (v1 - v3) * (i * DIR): forward multiplies by -i, inverse by +i
        const float2 s3 = DIR < 0 ? make_float2(dd.y, -dd.x) : make_float2(-dd.y, dd.x);
        const int j0 = ((lane - k) << 2) + k;
        dst[j0] = make_float2(s0.x + s2.x, s0.y + s2.y);
        dst[j0 + Ns] = make_float2(s1.x + s3.x, s1.y + s3.y);
        dst[j0 + 2 * Ns] = make_float2(s0.x - s2.x, s0.y - s2.y);
        dst[j0 + 3 * Ns] = make_float2(s1.x - s3.x, s1.y - s3.y);
        wave_lds_sync();   // each wave transforms its own frame in its own buffers
        float2* t = src; src = dst; dst = t;
    }
}

// twid = tw256[256] ++ tw512[256] (tw512[k] = exp(-2 pi i k / 512)), win[512] -> LDS; the caller's barrier publishes them
__device__ __forceinline__ void fft_tables_load(float2* s_tw, float2* s_tw512, float* s_win, const float2* twid,
                                                const float* win, int tid, int nthreads) {
    for (int i = tid; i < 256; i += nthreads) { s_tw[i] = twid[i]; s_tw512[i] = twid[256 + i]; }
    for (int i = tid; i < 512; i += nthreads) s_win[i] = win[i];
}

// ---- analysis: samples (2m, 2m+1) of a frame, windowed, are element m of the packed frame
__device__ __forceinline__ float2 frame_window(float2 c, const float* s_win, int m) {
    float2 v;
    v.x = c.x * s_win[2 * m];
    v.y = c.y * s_win[2 * m + 1];
    return v;
}
// real-FFT split: X[k] = Ze + exp(-2 pi i k/512) Zo, Ze = (Z[k]+conj(Z[256-k]))/2, Zo = (Z[k]-conj(Z[256-k]))/(2i);
// zk = A[k], which the caller holds for the Nyquist bin
__device__ __forceinline__ float2 rfft_bin(const float2* A, const float2* s_tw512, int k, float2 zk) {
    const float2 zm = A[(256 - k) & 255];
    const float2 ze = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
    const float2 zo = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
    const float2 r = cmul(s_tw512[k], zo);
    return make_float2(ze.x + r.x, ze.y + r.y);
}
// Nyquist bin: X[256] = Re Z[0] - Im Z[0]
__device__ __forceinline__ float2 rfft_nyquist(float2 z0) { return make_float2(z0.x - z0.y, 0.f); }

// ---- synthesis.  merge: Z[k] = Xe + i Xo, Xe = (X[k]+conj(X[256-k]))/2, Xo = (X[k]-conj(X[256-k]))/2 * exp(+2 pi i k/512);
// xk = X[k], xm = X[256-k].  c2r semantics: the imaginary parts of DC and Nyquist are ignored.
__device__ __forceinline__ float2 irfft_bin(float2 xk, float2 xm, const float2* s_tw512, int k) {
    xm.y = -xm.y;
    if (k == 0) { xk.y = 0.f; xm.y = 0.f; }
    const float2 xe = make_float2(0.5f * (xk.x + xm.x), 0.5f * (xk.y + xm.y));
    float2 w = s_tw512[k];
    w.y = -w.y;
    const float2 xo = cmul(make_float2(0.5f * (xk.x - xm.x), 0.5f * (xk.y - xm.y)), w);
    return make_float2(xe.x - xo.y, xe.y + xo.x);
}
// element m of the inverse transform -> samples (2m, 2m+1) of the windowed frame (the 256-point c2r scale, then win)
__device__ __forceinline__ float2 irfft_window(float2 z, const float* s_win, int m) {
    return make_float2((z.x * (1.0f / 256.0f)) * s_win[2 * m], (z.y * (1.0f / 256.0f)) * s_win[2 * m + 1]);
}
// overlap-add: sample i of a hop block is (frame j's 256 + i) + (frame j+1's i), over the two windows' squares
__device__ __forceinline__ float ola_env(const float* s_win, int i) {
    return s_win[256 + i] * s_win[256 + i] + s_win[i] * s_win[i];
}
__device__ __forceinline__ float ola_div(float acc, float env) { return env > 1e-11f ? acc / env : acc; }

// ---- reflect padding (center=True): sample i of the padded signal is sample reflect_idx(i, L) of the signal
__device__ __forceinline__ long reflect_idx(long i, long L) {
    long j = i - 256;
    j = j < 0 ? -j : j;
    return j >= L ? 2 * (L - 1) - j : j;
}
// samples of frame t: lane holds the pairs (2m, 2m+1), m = lane + 64 q.  A frame that lies inside the utterance's Lb
// samples and starts 8-byte aligned is read as one 8-byte load per pair; the others (the first and the last two of an
// utterance, or an odd row start) go through the reflection
__device__ __forceinline__ void frame_fetch(const float* x, int t, long Lb, int lane, float2 (&v)[4]) {
    const long lo = 256L * t - 256;                       // first sample of the frame in the unpadded signal
    if (lo >= 0 && lo + 512 <= Lb && ((reinterpret_cast<uintptr_t>(x + lo) & 7) == 0)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const float2*>(x + lo + 2 * (lane + 64 * q));
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long i0 = 256L * t + 2 * (lane + 64 * q);
            v[q] = make_float2(x[reflect_idx(i0, Lb)], x[reflect_idx(i0 + 1, Lb)]);
        }
    }
}

// ---- 16-bit PCM: x = s / 32768 (exact in fp32); s = clip(rint(y * 32768), -32768, 32767), round half to even
__device__ __forceinline__ float pcm16_widen(int s) { return (float)s * (1.0f / 32768.0f); }
__device__ __forceinline__ int pcm16_round(float y) {
    return (int)fminf(fmaxf(__builtin_rintf(y * 32768.0f), -32768.0f), 32767.0f);
}

}   // namespace gtfft
