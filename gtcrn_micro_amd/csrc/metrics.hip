// metrics.hip -- SDR, SI-SNR and STOI of (clean, enhanced) pairs, on the device ("scores" in include/gtcrn_micro_hip.h).
//
// Six launches per call, each clip in its own slice of the workspace:
//   k_score_moments   one workgroup per clip: means, centred sums, SI-SNR's projection and its residual (three passes)
//   k_score_resample  (tile of 256 outputs, clip, signal): the 5/8 polyphase stage, 16 kHz -> 10 kHz
//   k_score_energy    (8 frames, clip): windowed frame energies of ref in dB
//   k_score_mask      one workgroup per clip: maximum, keep mask, exclusive scan -> the list of kept frames
//   k_score_env       (4 frames, clip, signal): overlap-add of the kept frames gathered straight into the frame, window,
//                     512-point real FFT (one wave per frame), 15 third-octave band envelopes
//   k_score_stoi      one workgroup per clip: the 30-frame segment correlations and the record
// Every reduction is a fixed-order one that depends on the clip's own length alone: a thread's strided partial sum, then
// a tree over the workgroup; no atomics, no cross-workgroup reduction inside a launch (the launch boundary is the
// hand-off).  That is what makes a record's bits independent of B, the row, L and the neighbours' lengths.
// A NaN or Inf stays in its clip: every index comes from the clip's length and from counts of kept frames, never from a
// sample's value, and every store goes to the clip's own slice.
//
// gtcrn_score_ext ("scores, extended") runs the envelope chain and k_score_stoi as they are and adds, under the same rules:
//   k_score_ext_moments  k_score_moments' body, writing the head of a 64-byte record
//   k_score_estoi        (8 segments, clip): a 15 x 30 envelope pair per 32-lane half in registers, d_s per segment
//   k_score_segsnr       (32 frames, clip): both rows' samples of the run staged in LDS once, one wave per frame, v per frame
//   k_score_ext_finish   one workgroup per clip: the means of d_s and v, and the rest of the record
#include "metrics.h"

#include <cfloat>

#include "fft256.h"

namespace gtm {

namespace {

using namespace gtfft;

constexpr int TH = 256;
constexpr double SC_EPS = 2.220446049250313e-16;   // 2^-52

__device__ __forceinline__ int clip_len(const ScorePlan& p, int b) {
    long n = p.lens ? (long)p.lens[b] : p.L;
    n = n < 0 ? 0 : n;
    return (int)(n > p.L ? p.L : n);
}
__device__ __forceinline__ char* clip_ws(const ScorePlan& p, int b) { return p.ws + (long)b * p.lay.clip_bytes; }

// sum over the workgroup's 256 threads in a fixed tree; every thread gets the total
__device__ __forceinline__ double block_sum(double v, double* sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = TH / 2; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// ---- SDR / SI-SNR (eval_intrusive_metrics.py:74-91): fp32 samples, double sums, residuals formed sample by sample
// (one body for k_score_moments and k_score_ext_moments, which differ in the record they write)
__device__ __forceinline__ void clip_moments(const ScorePlan& p, int b, double* sh, double& sdr, double& sisnr) {
    const int tid = threadIdx.x;
    sdr = 0.0; sisnr = 0.0;
    if (p.what & 3) {
        const int n = clip_len(p, b);
        const float* r = p.ref + (long)b * p.ref_stride;
        const float* y = p.inf + (long)b * p.inf_stride;
        double sr = 0.0, sy = 0.0;
        for (int i = tid; i < n; i += TH) { sr += (double)r[i]; sy += (double)y[i]; }
        const double mr = block_sum(sr, sh) / (double)n, my = block_sum(sy, sh) / (double)n;
        double dot = 0.0, rr = 0.0, dd = 0.0;
        for (int i = tid; i < n; i += TH) {
            const double rc = (double)r[i] - mr, yc = (double)y[i] - my, d = yc - rc;
            dot += yc * rc; rr += rc * rc; dd += d * d;
        }
        dot = block_sum(dot, sh); rr = block_sum(rr, sh); dd = block_sum(dd, sh);
        sdr = 10.0 * log10((rr + 1e-8) / (dd + 1e-8));
        if (p.what & 2) {
            const double a = dot / (rr + (double)n * 1e-8);   // the reference's sum(ref^2 + 1e-8)
            double tt = 0.0, ee = 0.0;
            for (int i = tid; i < n; i += TH) {
                const double t = a * ((double)r[i] - mr), e = ((double)y[i] - my) - t;
                tt += t * t; ee += e * e;
            }
            tt = block_sum(tt, sh); ee = block_sum(ee, sh);
            sisnr = 10.0 * log10((tt + 1e-8) / (ee + 1e-8));
        }
    }
}

__global__ __launch_bounds__(TH) void k_score_moments(ScorePlan p) {
    __shared__ double sh[TH];
    const int b = blockIdx.x, tid = threadIdx.x;
    double sdr, sisnr;
    clip_moments(p, b, sh, sdr, sisnr);
    if (tid == 0) {
        ScoreRecord rec;
        rec.sdr = (p.what & 1) ? sdr : 0.0;
        rec.sisnr = (p.what & 2) ? sisnr : 0.0;
        rec.stoi = 0.0; rec.kept_frames = 0; rec.segments = 0;   // k_score_stoi fills these when STOI is asked for
        p.out[b] = rec;
    }
}

// ---- 16 kHz -> 10 kHz: y[j] = sum_i x[i] h[8 j - 5 i + 256], products exact in double, summed in ascending i
constexpr int RS_XS = 528;
__global__ __launch_bounds__(TH) void k_score_resample(ScorePlan p) {
    __shared__ float xs[RS_XS];
    __shared__ float hs[SC_NTAPS + 3];
    const int b = blockIdx.y, sig = blockIdx.z, tid = threadIdx.x;
    const int len = clip_len(p, b);
    const int n10 = (int)score_n10(len);
    const int j0 = blockIdx.x * TH;
    if (j0 >= n10) return;
    const float* x = sig ? p.inf + (long)b * p.inf_stride : p.ref + (long)b * p.ref_stride;
    // inputs the tile's outputs read: ceil((8 j0 - 256) / 5) .. floor((8 (j0 + 255) + 256) / 5), at most 512
    const int i_lo = (8 * j0 + 8) / 5 - 52, i_hi = (8 * (j0 + TH - 1) + 256) / 5;
    for (int t = tid; t <= i_hi - i_lo && t < RS_XS; t += TH) {
        const int i = i_lo + t;
        xs[t] = (i >= 0 && i < len) ? x[i] : 0.0f;
    }
    for (int t = tid; t < SC_NTAPS; t += TH) hs[t] = p.tab.taps[t];
    __syncthreads();
    const int j = j0 + tid;
    if (j >= n10) return;
    const int imin = (8 * j + 8) / 5 - 52, imax = (8 * j + 256) / 5;
    double acc = 0.0;
    for (int i = imin; i <= imax; ++i) acc += (double)xs[i - i_lo] * (double)hs[8 * j + 256 - 5 * i];
    float* y = reinterpret_cast<float*>(clip_ws(p, b) + p.lay.o_x10) + (long)sig * p.lay.x10_stride;
    y[j] = (float)acc;
}

// ---- e_j = 20 log10(||w ref_frame_j|| + EPS): one wave per frame, four samples per lane, double
constexpr int EN_FRAMES = 8;
__global__ __launch_bounds__(TH) void k_score_energy(ScorePlan p) {
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nfr = (int)score_frames_of(score_n10(clip_len(p, b)));
    const float* x = reinterpret_cast<const float*>(clip_ws(p, b) + p.lay.o_x10);
    double* edb = reinterpret_cast<double*>(clip_ws(p, b) + p.lay.o_edb);
    for (int q = 0; q < EN_FRAMES / 4; ++q) {
        const int f = blockIdx.x * EN_FRAMES + q * 4 + wv;
        if (f >= nfr) return;                                    // (wave-uniform; no workgroup barrier below)
        const float4 v = *reinterpret_cast<const float4*>(x + (long)f * SC_HOP + 4 * lane);
        const double* w = p.tab.win + 4 * lane;
        const double a0 = w[0] * (double)v.x, a1 = w[1] * (double)v.y, a2 = w[2] * (double)v.z, a3 = w[3] * (double)v.w;
        double acc = ((a0 * a0 + a1 * a1) + a2 * a2) + a3 * a3;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) edb[f] = 20.0 * log10(sqrt(acc) + SC_EPS);
    }
}

// ---- keep frame j iff e_j > max e - 40; kept[k] = the k-th kept frame.  k counts kept frames below j, so k <= j < nfr.
__global__ __launch_bounds__(TH) void k_score_mask(ScorePlan p) {
    __shared__ double sh[TH];
    __shared__ int cnt[TH / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int len = clip_len(p, b);
    const int n10 = (int)score_n10(len), nfr = (int)score_frames_of(n10);
    char* ws = clip_ws(p, b);
    const double* edb = reinterpret_cast<const double*>(ws + p.lay.o_edb);
    int* kept = reinterpret_cast<int*>(ws + p.lay.o_kept);
    int* flag = reinterpret_cast<int*>(ws + p.lay.o_flag);
    double m = -DBL_MAX;
    for (int f = tid; f < nfr; f += TH) { const double v = edb[f]; if (v > m) m = v; }   // a NaN never becomes the maximum
    sh[tid] = m;
    __syncthreads();
    for (int s = TH / 2; s > 0; s >>= 1) {
        if (tid < s && sh[tid + s] > sh[tid]) sh[tid] = sh[tid + s];
        __syncthreads();
    }
    const double thr = sh[0] - 40.0;
    int base = 0;
    for (int f0 = 0; f0 < nfr; f0 += TH) {
        const int f = f0 + tid;
        const bool keep = f < nfr && edb[f] > thr;
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) cnt[wv] = __popcll(bal);
        __syncthreads();
        int off = base, tot = 0;
        for (int w = 0; w < TH / 64; ++w) { if (w < wv) off += cnt[w]; tot += cnt[w]; }
        if (f < nfr) flag[f] = keep ? 1 : 0;
        if (keep) {
            const int k = off + __popcll(bal & ((1ull << lane) - 1ull));
            if (k < nfr) kept[k] = f;
        }
        base += tot;
        __syncthreads();
    }
    if (tid == 0) {
        int* h = reinterpret_cast<int*>(ws);
        const int K = base < nfr ? base : nfr;
        h[SC_H_LEN] = len; h[SC_H_N10] = n10; h[SC_H_NFR] = nfr; h[SC_H_K] = K; h[SC_H_M] = K > 0 ? K - 1 : 0;
    }
}

// ---- band envelopes.  Frame m of the overlap-added signal is gathered from the kept frames m - 1, m, m + 1 of the
// 10 kHz signal; 512 real samples (the upper 256 zero) are packed as 256 complex, radix-4 Stockham FFT in LDS (one wave
// per frame) and real split -- fft256<-1> and rfft_bin of fft256.h, which k_stft calls too -- then |X|^2, and one lane per
// band sums its bins in ascending order.
constexpr int ENV_WAVES = 4;
__global__ __launch_bounds__(ENV_WAVES * 64) void k_score_env(ScorePlan p) {
    __shared__ float2 s_tw[256];
    __shared__ float2 s_tw512[256];
    __shared__ float s_win[SC_FRAME];
    __shared__ int s_band[2 * SC_BANDS];
    __shared__ float2 s_buf[ENV_WAVES][2][256];
    const int b = blockIdx.y, sig = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int i = tid; i < 256; i += ENV_WAVES * 64) { s_tw[i] = p.tab.tw256[i]; s_tw512[i] = p.tab.tw512[i]; s_win[i] = p.tab.winf[i]; }
    if (tid < 2 * SC_BANDS) s_band[tid] = p.tab.bands[tid];
    __syncthreads();
    char* ws = clip_ws(p, b);
    const int* h = reinterpret_cast<const int*>(ws);
    const int K = h[SC_H_K], M = h[SC_H_M];
    const int m = blockIdx.x * ENV_WAVES + wv;
    if (m >= M) return;                                          // (wave-uniform; no workgroup barrier below)
    const int* kept = reinterpret_cast<const int*>(ws + p.lay.o_kept);
    const float* x = reinterpret_cast<const float*>(ws + p.lay.o_x10) + (long)sig * p.lay.x10_stride;
    float2* A = s_buf[wv][0];
    float2* Bf = s_buf[wv][1];
    // z[i] = w[i] ola[128 m + i], ola[128 q + r] = w[r + 128] x[s_(q-1) + r + 128] + w[r] x[s_q + r], s_q = 128 kept[q];
    // q = m or m + 1 <= M = K - 1, and kept[q] < nfr, so every sample read lies inside the clip's 10 kHz signal
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int n = lane + 64 * c;                             // the pair (2n, 2n + 1), n < 128
        float z[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int i = 2 * n + e, q = m + (i >> 7), r = i & 127;
            float v = 0.0f;
            if (q >= 1) v = s_win[r + 128] * x[(long)kept[q - 1] * SC_HOP + r + 128];
            if (q < K) v += s_win[r] * x[(long)kept[q] * SC_HOP + r];
            z[e] = s_win[i] * v;
        }
        A[n] = make_float2(z[0], z[1]);
        A[n + 128] = make_float2(0.0f, 0.0f);
    }
    wave_lds_sync();
    fft256<-1>(A, Bf, s_tw, lane);
    float* P = reinterpret_cast<float*>(Bf);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = lane + 64 * q;
        const float2 X = rfft_bin(A, s_tw512, k, A[k]);
        P[k] = X.x * X.x + X.y * X.y;
    }
    wave_lds_sync();
    if (lane < SC_BANDS) {
        double acc = 0.0;
        for (int k = s_band[lane]; k < s_band[SC_BANDS + lane]; ++k) acc += (double)P[k];
        float* env = reinterpret_cast<float*>(ws + p.lay.o_env) + ((long)sig * SC_BANDS + lane) * p.lay.env_stride;
        env[m] = (float)sqrt(acc);
    }
}

// ---- STOI: one (band, segment) pair per thread and turn, in double; d summed over pairs in a fixed order
__global__ __launch_bounds__(TH) void k_score_stoi(ScorePlan p) {
    __shared__ double sh[TH];
    const int b = blockIdx.x, tid = threadIdx.x;
    const char* ws = clip_ws(p, b);
    const int* h = reinterpret_cast<const int*>(ws);
    const int K = h[SC_H_K], M = h[SC_H_M];
    const int S = M >= SC_SEG ? M - SC_SEG + 1 : 0;
    double stoi = 1e-5;
    if (S > 0) {
        const float* er = reinterpret_cast<const float*>(ws + p.lay.o_env);
        const float* ei = er + (long)SC_BANDS * p.lay.env_stride;
        const double clipc = 1.0 + 5.623413251903491;            // 1 + 10^(15/20)
        double part = 0.0;
        for (int it = tid; it < SC_BANDS * S; it += TH) {
            const int j = it / S, s = it - j * S;
            const float* xr = er + (long)j * p.lay.env_stride + s;
            const float* yr = ei + (long)j * p.lay.env_stride + s;
            double x[SC_SEG], y[SC_SEG];
            double sxx = 0.0, syy = 0.0;
#pragma unroll
            for (int t = 0; t < SC_SEG; ++t) { x[t] = (double)xr[t]; y[t] = (double)yr[t]; sxx += x[t] * x[t]; syy += y[t] * y[t]; }
            const double alpha = sqrt(sxx) / (sqrt(syy) + SC_EPS);
            double mx = 0.0, my = 0.0;
#pragma unroll
            for (int t = 0; t < SC_SEG; ++t) {
                const double a = alpha * y[t], c = x[t] * clipc;
                y[t] = a < c ? a : c;
                mx += x[t]; my += y[t];
            }
            mx /= (double)SC_SEG; my /= (double)SC_SEG;
            double nx = 0.0, ny = 0.0;
#pragma unroll
            for (int t = 0; t < SC_SEG; ++t) { x[t] -= mx; y[t] -= my; nx += x[t] * x[t]; ny += y[t] * y[t]; }
            nx = sqrt(nx) + SC_EPS; ny = sqrt(ny) + SC_EPS;
            double d = 0.0;
#pragma unroll
            for (int t = 0; t < SC_SEG; ++t) d += (x[t] / nx) * (y[t] / ny);
            part += d;
        }
        stoi = block_sum(part, sh) / (double)(SC_BANDS * S);
    }
    if (tid == 0) {
        p.out[b].stoi = stoi;
        p.out[b].kept_frames = K;
        p.out[b].segments = S;
    }
}

// ---- gtcrn_score_ext.  The envelope chain and k_score_stoi above run unchanged on p.base (k_score_stoi's 32-byte records
// go to the head of the ext workspace); the kernels below write SDR / SI-SNR into the 64-byte record, add ESTOI and
// segmental SNR per segment / frame in the clip's slice, and finish the record.

// k_score_moments with the 64-byte record: SDR and SI-SNR by the same body, everything behind them 0
__global__ __launch_bounds__(TH) void k_score_ext_moments(ScoreExtPlan p) {
    __shared__ double sh[TH];
    const int b = blockIdx.x;
    double sdr, sisnr;
    clip_moments(p.base, b, sh, sdr, sisnr);
    if (threadIdx.x == 0) {
        ScoreExtRecord rec = {};
        rec.base.sdr = (p.what & 1) ? sdr : 0.0;
        rec.base.sisnr = (p.what & 2) ? sisnr : 0.0;
        p.out[b] = rec;
    }
}

// sum over a 32-lane half of the wave in a fixed butterfly; every lane of the half gets the same bits
// (the four steps inside a row of 16 lanes are DPP moves -- lane ^ 1, lane ^ 2, then the mirror of 8 and of 16 lanes, whose
// partner lies in the other, already uniform, group -- so that only the last step goes through the LDS crossbar)
template <int CTRL>
__device__ __forceinline__ double dpp_move(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double half_sum(double v) {
    v += dpp_move<0xB1>(v);      // quad_perm [1, 0, 3, 2]
    v += dpp_move<0x4E>(v);      // quad_perm [2, 3, 0, 1]
    v += dpp_move<0x141>(v);     // row_half_mirror
    v += dpp_move<0x140>(v);     // row_mirror
    v += __shfl_xor(v, 16, 64);
    return v;
}

// ESTOI: one segment per 32-lane half, one frame column per lane (lanes 30, 31 of a half and halves without a segment hold
// zeros, which every sum ignores); the 15 x 30 pair stays in registers.  d_s depends on nothing but the segment.
__global__ __launch_bounds__(SX_SEGS_PER_WG * 32) void k_score_estoi(ScoreExtPlan p) {
    const int b = blockIdx.y, tid = threadIdx.x, t = tid & 31;
    char* ws = clip_ws(p.base, b);
    const int M = reinterpret_cast<const int*>(ws)[SC_H_M];
    const int S = M >= SC_SEG ? M - SC_SEG + 1 : 0;
    const int s = blockIdx.x * SX_SEGS_PER_WG + (tid >> 5);
    if (blockIdx.x * SX_SEGS_PER_WG >= S) return;                // (workgroup-uniform)
    const bool live = s < S && t < SC_SEG;                       // s + t <= S - 1 + 29 = M - 1
    const float* er = reinterpret_cast<const float*>(ws + p.base.lay.o_env);
    const float* ei = er + (long)SC_BANDS * p.base.lay.env_stride;
    double x[SC_BANDS], y[SC_BANDS];
#pragma unroll
    for (int j = 0; j < SC_BANDS; ++j) {
        x[j] = live ? (double)er[(long)j * p.base.lay.env_stride + s + t] : 0.0;
        y[j] = live ? (double)ei[(long)j * p.base.lay.env_stride + s + t] : 0.0;
    }
    // rows: a band's 30 values lose their mean and are divided by (their norm + EPS).  A double division costs some
    // forty instructions, so a denominator shared by many values is inverted once (1 / 30 and 1 / 15 are constants).
    constexpr double INV_SEG = 1.0 / (double)SC_SEG, INV_BANDS = 1.0 / (double)SC_BANDS;
#pragma unroll
    for (int j = 0; j < SC_BANDS; ++j) {
        const double mx = half_sum(x[j]) * INV_SEG, my = half_sum(y[j]) * INV_SEG;
        const double xc = live ? x[j] - mx : 0.0, yc = live ? y[j] - my : 0.0;
        const double ix = 1.0 / (sqrt(half_sum(xc * xc)) + SC_EPS), iy = 1.0 / (sqrt(half_sum(yc * yc)) + SC_EPS);
        x[j] = xc * ix;
        y[j] = yc * iy;
    }
    // columns: a frame's 15 values, the same way, in the lane; sum (x / nx) (y / ny) = (sum x y) / (nx ny)
    double mx = 0.0, my = 0.0;
#pragma unroll
    for (int j = 0; j < SC_BANDS; ++j) { mx += x[j]; my += y[j]; }
    mx *= INV_BANDS; my *= INV_BANDS;
    double nx = 0.0, ny = 0.0, d = 0.0;
#pragma unroll
    for (int j = 0; j < SC_BANDS; ++j) { x[j] -= mx; y[j] -= my; nx += x[j] * x[j]; ny += y[j] * y[j]; d += x[j] * y[j]; }
    d /= (sqrt(nx) + SC_EPS) * (sqrt(ny) + SC_EPS);
    d = half_sum(live ? d : 0.0);
    if (t == 0 && s < S) reinterpret_cast<double*>(ws + p.o_ds)[s] = d / (double)SC_SEG;
}

// Segmental SNR: a workgroup stages the samples of its SX_RUN consecutive frames of both rows once, a wave takes every
// fourth frame: lane i holds samples i, i + 64, ... of the frame (and their window values, the same for every frame).
constexpr int SX_WAVES = 4;
constexpr int SX_SPAN = (SX_RUN - 1) * SX_HOP + SX_FRAME;         // samples a run reads
constexpr int SX_PER_LANE = (SX_FRAME + 63) / 64;
__global__ __launch_bounds__(SX_WAVES * 64) void k_score_segsnr(ScoreExtPlan p) {
    __shared__ float rs[SX_SPAN];
    __shared__ float ys[SX_SPAN];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = clip_len(p.base, b);
    const int F = (int)score_segsnr_frames_of(n);
    const int f0 = blockIdx.x * SX_RUN;
    if (f0 >= F) return;                                         // (workgroup-uniform)
    const float* r = p.base.ref + (long)b * p.base.ref_stride;
    const float* y = p.base.inf + (long)b * p.base.inf_stride;
    const int i0 = f0 * SX_HOP;
    for (int i = tid; i < SX_SPAN; i += SX_WAVES * 64) {         // a frame that exists reads below n; the rest is never used
        const bool in = i0 + i < n;
        rs[i] = in ? r[i0 + i] : 0.0f;
        ys[i] = in ? y[i0 + i] : 0.0f;
    }
    double w[SX_PER_LANE];
#pragma unroll
    for (int k = 0; k < SX_PER_LANE; ++k) w[k] = lane + 64 * k < SX_FRAME ? p.w480[lane + 64 * k] : 0.0;
    __syncthreads();
    double* v = reinterpret_cast<double*>(clip_ws(p.base, b) + p.o_v);
    for (int q = wv; q < SX_RUN; q += SX_WAVES) {
        const int f = f0 + q;
        if (f >= F) break;                                       // (wave-uniform; no workgroup barrier below)
        double num = 0.0, den = 0.0;
#pragma unroll
        for (int k = 0; k < SX_PER_LANE; ++k) {
            const int i = lane + 64 * k;
            if (i < SX_FRAME) {
                const double rv = (double)rs[q * SX_HOP + i], e = rv - (double)ys[q * SX_HOP + i];
                const double a = w[k] * rv, c = w[k] * e;
                num += a * a; den += c * c;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { num += __shfl_xor(num, o, 64); den += __shfl_xor(den, o, 64); }
        if (lane == 0) {
            const double db = 10.0 * log10(num / (den + SC_EPS) + SC_EPS);
            v[f] = db < -10.0 ? -10.0 : db > 35.0 ? 35.0 : db;   // (a NaN stays a NaN)
        }
    }
}

// Finish: one workgroup per clip sums its d_s and its v (a thread's strided partial, then the tree) and writes the record.
__global__ __launch_bounds__(TH) void k_score_ext_finish(ScoreExtPlan p) {
    __shared__ double sh[TH];
    const int b = blockIdx.x, tid = threadIdx.x;
    const char* ws = clip_ws(p.base, b);
    int K = 0, S = 0, F = 0;
    double estoi = 0.0, segsnr = 0.0;
    if (p.what & 12) {
        const int* h = reinterpret_cast<const int*>(ws);
        const int M = h[SC_H_M];
        K = h[SC_H_K];
        S = M >= SC_SEG ? M - SC_SEG + 1 : 0;
    }
    if (p.what & 8) {
        estoi = 1e-5;
        if (S > 0) {
            const double* d = reinterpret_cast<const double*>(ws + p.o_ds);
            double part = 0.0;
            for (int s = tid; s < S; s += TH) part += d[s];
            estoi = block_sum(part, sh) / (double)S;
        }
    }
    if (p.what & 16) {
        F = (int)score_segsnr_frames_of(clip_len(p.base, b));
        const double* v = reinterpret_cast<const double*>(ws + p.o_v);
        double part = 0.0;
        for (int f = tid; f < F; f += TH) part += v[f];
        segsnr = block_sum(part, sh) / (double)F;                // F = 0: 0 / 0 = NaN, as SDR for n = 0
    }
    if (tid == 0) {                                              // (k_score_ext_moments wrote SDR, SI-SNR and the zeros)
        ScoreExtRecord* rec = p.out + b;
        if (p.what & 4) rec->base.stoi = p.base.out[b].stoi;     // k_score_stoi's 32-byte record in the workspace
        if (p.what & 12) { rec->base.kept_frames = K; rec->base.segments = S; }
        rec->estoi = estoi; rec->segsnr = segsnr; rec->segsnr_frames = F;
    }
}

template <typename T>
__global__ void k_score_debug_cvt(const T* __restrict__ src, float* __restrict__ dst, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (float)src[i];
}

}  // namespace

ScoreLayout score_layout(long L) {
    auto up = [](long bytes) { return (bytes + 63) & ~63L; };
    ScoreLayout y;
    y.n10 = score_n10(L);
    y.nfr = score_frames_of(y.n10);
    y.x10_stride = (y.n10 + 15) & ~15L;
    y.env_stride = ((y.nfr > 1 ? y.nfr - 1 : 1) + 15) & ~15L;
    long o = SC_H_WORDS * (long)sizeof(int);
    y.o_x10 = o = up(o);   o += 2 * y.x10_stride * (long)sizeof(float);
    y.o_edb = o = up(o);   o += (y.nfr + 1) * (long)sizeof(double);
    y.o_kept = o = up(o);  o += (y.nfr + 1) * (long)sizeof(int);
    y.o_flag = o = up(o);  o += (y.nfr + 1) * (long)sizeof(int);
    y.o_env = o = up(o);   o += 2L * SC_BANDS * y.env_stride * (long)sizeof(float);
    y.clip_bytes = up(o);
    return y;
}

const char* score_stage_name(int i) {
    static const char* const names[SC_STAGES] = {"k_score_moments", "k_score_resample", "k_score_energy", "k_score_mask",
                                                 "k_score_env", "k_score_stoi"};
    return i >= 0 && i < SC_STAGES ? names[i] : "";
}

int launch_score(const ScorePlan& p, hipStream_t s, hipEvent_t* ev) {
    auto mark = [&](int i) { if (ev) (void)hipEventRecord(ev[i], s); };
    const unsigned B = (unsigned)p.B;
    mark(0);
    hipLaunchKernelGGL(k_score_moments, dim3(B), dim3(TH), 0, s, p);
    mark(1);
    if (p.what & 4) {
        const long n10 = p.lay.n10, nfr = p.lay.nfr, M = nfr > 1 ? nfr - 1 : 0;
        hipLaunchKernelGGL(k_score_resample, dim3((unsigned)((n10 + TH - 1) / TH), B, 2), dim3(TH), 0, s, p);
        mark(2);
        if (nfr > 0) hipLaunchKernelGGL(k_score_energy, dim3((unsigned)((nfr + EN_FRAMES - 1) / EN_FRAMES), B), dim3(TH), 0, s, p);
        mark(3);
        hipLaunchKernelGGL(k_score_mask, dim3(B), dim3(TH), 0, s, p);
        mark(4);
        if (M > 0) hipLaunchKernelGGL(k_score_env, dim3((unsigned)((M + ENV_WAVES - 1) / ENV_WAVES), B, 2), dim3(ENV_WAVES * 64), 0, s, p);
        mark(5);
        hipLaunchKernelGGL(k_score_stoi, dim3(B), dim3(TH), 0, s, p);
        mark(6);
    } else if (ev) {
        for (int i = 2; i <= SC_STAGES; ++i) mark(i);
    }
    return (int)hipGetLastError();
}

ScoreExtPlan score_ext_layout(long L) {
    auto up = [](long bytes) { return (bytes + 63) & ~63L; };
    ScoreExtPlan x;
    x.base.lay = score_layout(L);
    const long M = x.base.lay.nfr > 1 ? x.base.lay.nfr - 1 : 0;
    x.max_segments = M >= SC_SEG ? M - SC_SEG + 1 : 0;
    x.max_frames = score_segsnr_frames_of(L);
    long o = x.base.lay.clip_bytes;
    x.o_ds = o;  o += up((x.max_segments + 1) * (long)sizeof(double));
    x.o_v = o;   o += up((x.max_frames + 1) * (long)sizeof(double));
    x.base.lay.clip_bytes = o;
    return x;
}

const char* score_ext_stage_name(int i) {
    static const char* const names[SX_STAGES] = {"k_score_ext_moments", "k_score_resample", "k_score_energy", "k_score_mask", "k_score_env",
                                                 "k_score_stoi", "k_score_estoi", "k_score_segsnr", "k_score_ext_finish"};
    return i >= 0 && i < SX_STAGES ? names[i] : "";
}

int launch_score_ext(const ScoreExtPlan& x, hipStream_t s, hipEvent_t* ev) {
    auto mark = [&](int i) { if (ev) (void)hipEventRecord(ev[i], s); };
    const ScorePlan& p = x.base;
    const unsigned B = (unsigned)p.B;
    mark(0);
    hipLaunchKernelGGL(k_score_ext_moments, dim3(B), dim3(TH), 0, s, x);
    mark(1);
    const long n10 = p.lay.n10, nfr = p.lay.nfr, M = nfr > 1 ? nfr - 1 : 0;
    if (x.what & 12) {
        hipLaunchKernelGGL(k_score_resample, dim3((unsigned)((n10 + TH - 1) / TH), B, 2), dim3(TH), 0, s, p);
        mark(2);
        if (nfr > 0) hipLaunchKernelGGL(k_score_energy, dim3((unsigned)((nfr + EN_FRAMES - 1) / EN_FRAMES), B), dim3(TH), 0, s, p);
        mark(3);
        hipLaunchKernelGGL(k_score_mask, dim3(B), dim3(TH), 0, s, p);
        mark(4);
        if (M > 0) hipLaunchKernelGGL(k_score_env, dim3((unsigned)((M + ENV_WAVES - 1) / ENV_WAVES), B, 2), dim3(ENV_WAVES * 64), 0, s, p);
    } else {
        mark(2); mark(3); mark(4);
    }
    mark(5);
    if (x.what & 4) hipLaunchKernelGGL(k_score_stoi, dim3(B), dim3(TH), 0, s, p);
    mark(6);
    if ((x.what & 8) && x.max_segments > 0)
        hipLaunchKernelGGL(k_score_estoi, dim3((unsigned)((x.max_segments + SX_SEGS_PER_WG - 1) / SX_SEGS_PER_WG), B), dim3(SX_SEGS_PER_WG * 32), 0, s, x);
    mark(7);
    if ((x.what & 16) && x.max_frames > 0)
        hipLaunchKernelGGL(k_score_segsnr, dim3((unsigned)((x.max_frames + SX_RUN - 1) / SX_RUN), B), dim3(SX_WAVES * 64), 0, s, x);
    mark(8);
    if (x.what & 28) hipLaunchKernelGGL(k_score_ext_finish, dim3(B), dim3(TH), 0, s, x);
    mark(9);
    return (int)hipGetLastError();
}

int launch_score_debug_cvt(const void* src, int kind, float* dst, long n, hipStream_t s) {
    if (n <= 0) return 0;
    const dim3 g((unsigned)((n + 255) / 256)), t(256);
    if (kind == 0) hipLaunchKernelGGL(k_score_debug_cvt<double>, g, t, 0, s, static_cast<const double*>(src), dst, n);
    else hipLaunchKernelGGL(k_score_debug_cvt<int>, g, t, 0, s, static_cast<const int*>(src), dst, n);
    return (int)hipGetLastError();
}

}  // namespace gtm
