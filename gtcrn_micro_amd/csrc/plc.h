// plc.h -- packet loss concealment ("packet loss concealment" in include/gtcrn_micro_hip.h).  The four
// cases of the contract as one set of __host__ __device__ functions (plc.hip runs them a wave per row on the device,
// plc_host.cpp a loop per row on the host for gtcrn_plc_rows_host), the argument record both share and the launch interface
// of plc.hip.  Both files are compiled with -ffp-contract=off: everything here is integer arithmetic but for the score (one
// rounded product and one rounded quotient in double) and the float cross-fade (three rounded fp32 operations).
#pragma once
#include "phone.h"     // gtp::dot2 / gtp::pack2 / gtp::pcm_of, and through it kernels.h: gtk::g711_encode / gtk::g711_decode

namespace gtl {

constexpr int MAX_N = 1024, MAX_LH = 1680, MAX_FADE_MS = 200, WAVES = 4, LANES = 64, THREADS = WAVES * LANES;
constexpr int NO_LAG = 0x7fffffff;

struct Record { int pos, lag, erased, events; };          // == one record of d_rec, 16 bytes
struct Prm { int pmin, pmax, W, D, T0, T1, F, fs; };      // == the 8 parameter words

struct PlcArgs {
    void* x;                   // M rows of n samples (float, int16 or G.711 codes) at stride
    long stride, hist_stride;
    const int* slots;          // [M], may be null: row i is stream i
    const int* lost;           // [M]
    const int* count;          // may be null
    short* hist;               // S histories at hist_stride
    Record* rec;               // [S]
    const int* params;         // [8]
    int M, n, S, law;
};

// ---- the tables ---------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int live_rows(int M, const int* count) {
    if (!count) return M;
    const int k = *count;
    return k < 0 ? 0 : (k < M ? k : M);
}
__host__ __device__ inline int slot_of(const int* slots, int row, int S) {
    const int s = slots ? slots[row] : row;
    return s >= 0 && s < S ? s : -1;
}
__host__ __device__ inline Prm prm_of(const int* w) { return {w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]}; }
__host__ __device__ inline int hist_len(Prm p) { return p.pmax + p.W; }
// Words that gtcrn_plc_params_host did not make turn the call into a no-op unless they keep every index inside a history.
__host__ __device__ inline bool prm_ok(Prm p, long hist_stride) {
    return p.pmin >= 1 && p.pmax >= p.pmin && p.pmax <= MAX_LH && p.W >= 1 && p.W <= MAX_LH && p.D >= 1 && hist_len(p) <= MAX_LH &&
           hist_len(p) <= hist_stride && p.T0 >= 0 && p.T0 <= (1 << 16) && p.T1 >= 1 && p.T1 <= (1 << 16) && p.F >= 1;
}
// A record as the cases see it: a zeroed record is a fresh stream; anything a call did not write is brought into range.
__host__ __device__ inline Record record_of(Record r, Prm p) {
    const int top = p.T0 + p.T1;
    return {r.pos >= 0 && r.pos < hist_len(p) ? r.pos : 0, r.lag < p.pmin ? p.pmin : (r.lag > p.pmax ? p.pmax : r.lag),
            r.erased < 0 ? 0 : (r.erased > top ? top : r.erased), r.events};
}
// Logical sample j (0 the oldest, Lh - 1 the newest) of a ring whose write position is pos; also where the j-th sample of an
// appended row goes (j may exceed Lh: the row then laps the ring).
__host__ __device__ inline int ring_at(int pos, int j, int Lh) { return (pos + j) % Lh; }
// The first sample of an appended row that is kept: a row longer than the history leaves only its last Lh samples.
__host__ __device__ inline int first_kept(int n, int Lh) { return n > Lh ? n - Lh : 0; }

// ---- samples ------------------------------------------------------------------------------------------------------------------
typedef unsigned char code_t;
__host__ __device__ inline int sample_in(float v, int) { return gtp::pcm_of(v); }
__host__ __device__ inline int sample_in(short v, int) { return v; }
__host__ __device__ inline int sample_in(code_t v, int law) { return gtk::g711_decode(law, v); }
__host__ __device__ inline void sample_out(float* dst, int o, int) { *dst = (float)o * 3.0517578125e-05f; }   // exact
__host__ __device__ inline void sample_out(short* dst, int o, int) { *dst = (short)o; }
__host__ __device__ inline void sample_out(code_t* dst, int o, int law) { *dst = (code_t)gtk::g711_encode(law, o); }

// ---- case 2: the lag ----------------------------------------------------------------------------------------------------------
__host__ __device__ inline int abs16(int v) { return v < 0 ? -v : v; }
__host__ __device__ inline int analysis_shift(int m) {
    const int bits = m > 0 ? 32 - __builtin_clz((unsigned)m) : 0;
    return bits > 10 ? bits - 10 : 0;
}
// c(p) and e(p) over i = 0, d, 2d, ... < W on the shifted history a[0 .. L); two terms a dot2.  |a| < 2^10 and at most 960
// terms, so neither sum reaches 2^30.  The lowest index read is L - W - p >= 0 for p <= pmax.
__host__ __device__ inline void corr_at(const short* a, int L, int p, int d, int W, int* c, int* e) {
    int cc = 0, ee = 0, i = 0;
    for (; i + d < W; i += 2 * d) {
        const uint32_t x = gtp::pack2(a[L - 1 - i], a[L - 1 - i - d]);
        const uint32_t y = gtp::pack2(a[L - 1 - i - p], a[L - 1 - i - d - p]);
        cc = gtp::dot2(x, y, cc);
        ee = gtp::dot2(y, y, ee);
    }
    if (i < W) {
        const uint32_t x = gtp::pack2(a[L - 1 - i], 0), y = gtp::pack2(a[L - 1 - i - p], 0);
        cc = gtp::dot2(x, y, cc);
        ee = gtp::dot2(y, y, ee);
    }
    *c = cc;
    *e = ee;
}
__host__ __device__ inline double score(int c, int e) {
    if (!(c > 0 && e > 0)) return 0.0;
    const double cc = (double)c * (double)c;
    return cc / (double)e;
}
__host__ __device__ inline double score_at(const short* a, int L, int p, int d, int W) {
    int c, e;
    corr_at(a, L, p, d, W, &c, &e);
    return score(c, e);
}
// The order of a search: a candidate (score s at lag p) replaces the best so far (bs at bp; bp = NO_LAG: none yet) when its
// score is positive and larger, or equal at a smaller lag.  A total order, so the order of the comparisons cannot matter.
__host__ __device__ inline bool better(double s, int p, double bs, int bp) { return s > 0.0 && (s > bs || (s == bs && p < bp)); }
// The refinement's range around the coarse winner p0.
__host__ __device__ inline int refine_lo(int p0, Prm p) { return p0 - p.D + 1 < p.pmin ? p.pmin : p0 - p.D + 1; }
__host__ __device__ inline int refine_hi(int p0, Prm p) { return p0 + p.D - 1 > p.pmax ? p.pmax : p0 + p.D - 1; }

// ---- cases 3 and 4 ------------------------------------------------------------------------------------------------------------
// g(t) on the scale 32768 = 1.
__host__ __device__ inline int fade_gain(int t, Prm p) {
    if (t < p.T0) return 32768;
    if (t - p.T0 >= p.T1) return 0;
    return 32768 - (int)(((unsigned)(t - p.T0) * 32768u) / (unsigned)p.T1);        // (T1 - 1) 2^15 < 2^31
}
// s[i] of a history h[0 .. Lh) in logical order at lag P, and the attenuated sample at time t.
__host__ __device__ inline int synth(const short* h, int Lh, int P, int i) { return h[Lh - P + i % P]; }
__host__ __device__ inline int attenuated(int s, int t, Prm p) { return (s * fade_gain(t, p) + 16384) >> 15; }
// r_i of a cross-fade over f samples.
__host__ __device__ inline int recover_ramp(int i, int f) { return ((i + 1) * 32768) / f; }
__host__ __device__ inline int recover_int(int x, int sa, int r) { return (x * r + sa * (32768 - r) + 16384) >> 15; }
__host__ __device__ inline void recover(float* x, int sa, int r, int) {
    const float rf = (float)r * 3.0517578125e-05f, saf = (float)sa * 3.0517578125e-05f;
    const float a = *x * rf, b = saf * (1.0f - rf);
    *x = a + b;
}
__host__ __device__ inline void recover(short* x, int sa, int r, int) { *x = (short)recover_int(*x, sa, r); }
__host__ __device__ inline void recover(code_t* x, int sa, int r, int law) {
    *x = (code_t)gtk::g711_encode(law, recover_int(gtk::g711_decode(law, *x), sa, r));
}
__host__ __device__ inline int saturate_erased(int erased, int n, Prm p) {
    const int top = p.T0 + p.T1;
    return erased + n > top ? top : erased + n;
}
// events: erasures in the low half, lost packets in the high half, each modulo 65536.
__host__ __device__ inline int events_next(int ev, bool begins) {
    const unsigned lo = ((unsigned)ev + (begins ? 1u : 0u)) & 0xFFFFu, hi = (((unsigned)ev >> 16) + 1u) & 0xFFFFu;
    return (int)(lo | (hi << 16));
}

// plc.hip
int launch_plc(const PlcArgs& a, int kind, hipStream_t s);       // kind 0 float, 1 int16, 2 G.711 codes
int launch_plc_reset(short* hist, long hist_stride, Record* rec, int S, const int* params, const int* slots, int M,
                     const int* count, hipStream_t s);

}  // namespace gtl
