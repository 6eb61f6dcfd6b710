// batch.hip -- training batches from a resident corpus: the plan, the pairs draw and the three passes of the mix draw
// (contract: include/gtcrn_micro_hip.h, "training batches from a resident corpus"), and the three
// passes of the mix at an SNR of active levels ("active levels"; section 7o) behind them.
//
// Compiled with -ffp-contract=off: every float and double operation below rounds once, as the contract states it, so
// numpy restates the output bit for bit.  The three sums of an item are 64-bit integers over its int16 samples: exact,
// hence independent of how the window is cut into chunks, and every workgroup of the later passes re-derives the very
// same gains from the very same partials.
//
// Shape of every draw kernel: 256 threads, a thread handles 8 consecutive output samples at a time (16 bytes of int16
// in, two 16-byte stores per output row out).  A window starts at any int16 index, so the 16-byte load is unaligned
// (the hardware splits it; a wave's lanes together still cover whole lines).  Only a group that touches the end of the
// speech clip, the wrap of the noise or the end of the row goes sample by sample.
#include "batch.h"

namespace gtb {

namespace {

constexpr float kScale = 3.0517578125e-05f;   // 2^-15: int16 * 2^-15 == int16 / 32768, exact

struct View {                  // item b as the draw kernels see it; every field clamped so that no read leaves its clip
    const short* s;            // speech (pairs: noisy) clip
    const short* n;            // noise (pairs: clean) clip
    long long len_s;
    unsigned len_n;
    long long sstart;
    unsigned nstart;
    float snr_amp, lvl_amp;
};

__device__ inline View view_of(const DrawArgs& d, int b, bool pairs) {
    const Item it = d.plan[b];
    View v;
    const int sc = clampi(it.sclip, 0, d.a.n - 1);
    const long long o0 = d.a.off[sc], o1 = d.a.off[sc + 1];
    v.s = d.a.pcm + o0;
    v.len_s = o1 > o0 ? o1 - o0 : 0;
    v.sstart = it.sstart > 0 ? it.sstart : 0;
    if (pairs) {
        v.n = d.b.pcm + o0;
        v.len_n = 0;
        v.nstart = 0;
    } else {
        const int nc = clampi(it.nclip, 0, d.b.n - 1);
        const long long n0 = d.b.off[nc], n1 = d.b.off[nc + 1];
        v.n = d.b.pcm + n0;
        const long long ln = n1 - n0;
        v.len_n = ln > 0 && ln <= 0x7fffffffLL ? (unsigned)ln : 0u;
        v.nstart = v.len_n ? (unsigned)it.nstart % v.len_n : 0u;
    }
    v.snr_amp = it.snr_amp;
    v.lvl_amp = it.lvl_amp;
    return v;
}

// 8 samples of a clip from `pos` on, zero past its end; samples at or beyond `cnt` (the end of the row) are zero too
__device__ inline void load_clip8(const short* p, long long len, long long pos, int cnt, int* x) {
    if (pos + GROUP <= len) {
        short t[GROUP];
        __builtin_memcpy(t, p + pos, sizeof(t));
#pragma unroll
        for (int k = 0; k < GROUP; ++k) x[k] = t[k];
    } else {
#pragma unroll
        for (int k = 0; k < GROUP; ++k) x[k] = pos + k < len ? (int)p[pos + k] : 0;
    }
    if (cnt < GROUP) {
#pragma unroll
        for (int k = 0; k < GROUP; ++k) x[k] = k < cnt ? x[k] : 0;
    }
}

// 8 samples of a wrapping clip: sample k is p[(j + k) mod len], j < len
__device__ inline void load_wrap8(const short* p, unsigned len, unsigned j, int cnt, int* x) {
    if (len == 0) {
#pragma unroll
        for (int k = 0; k < GROUP; ++k) x[k] = 0;
        return;
    }
    if ((unsigned long long)j + GROUP <= len) {
        short t[GROUP];
        __builtin_memcpy(t, p + j, sizeof(t));
#pragma unroll
        for (int k = 0; k < GROUP; ++k) x[k] = t[k];
    } else {
#pragma unroll
        for (int k = 0; k < GROUP; ++k) {
            x[k] = p[j];
            j = j + 1 == len ? 0u : j + 1;
        }
    }
    if (cnt < GROUP) {
#pragma unroll
        for (int k = 0; k < GROUP; ++k) x[k] = k < cnt ? x[k] : 0;
    }
}

__device__ inline unsigned wrap_index(const View& v, long i0) {      // (nstart + i0) mod len_n; both below 2^31
    return v.len_n ? (unsigned)(v.nstart + (unsigned)i0) % v.len_n : 0u;
}

// A workgroup's sum or maximum, returned to every thread.  sm: THREADS / 64 values.
template <typename T, bool MAX>
__device__ inline T block_all(T v, T* sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T w = __shfl_xor(v, o, 64);
        v = MAX ? (w > v ? w : v) : v + w;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = sm[0];
#pragma unroll
    for (int k = 1; k < THREADS / 64; ++k) r = MAX ? (sm[k] > r ? sm[k] : r) : r + sm[k];
    return r;
}

struct Sums { long long ss, sn, ssn; };

// an item's three sums from its chunks' partials (chunks <= THREADS)
__device__ inline Sums item_sums(const long long* part, int chunks, long long* sm) {
    long long a = 0, b = 0, c = 0;
    if ((int)threadIdx.x < chunks) {
        a = part[3 * threadIdx.x];
        b = part[3 * threadIdx.x + 1];
        c = part[3 * threadIdx.x + 2];
    }
    Sums s;
    s.ss = block_all<long long, false>(a, sm);
    s.sn = block_all<long long, false>(b, sm);
    s.ssn = block_all<long long, false>(c, sm);
    return s;
}

__device__ inline float noise_gain(const Sums& s, float snr_amp, int* flags) {
    if (s.sn == 0) { *flags |= FLAG_NOISE_ZERO; return 0.0f; }
    if (s.ss == 0) { *flags |= FLAG_SPEECH_ZERO; return 1.0f; }
    return (float)(sqrt((double)s.ss / (double)s.sn) * (double)snr_amp);
}

__device__ inline float level_gain(const Sums& s, float gn, float peak, float lvl_amp, long L, int* flags) {
    const double g = (double)gn;
    double sm = (double)s.ss + g * (2.0 * (double)s.ssn + g * (double)s.sn);
    if (!(sm > 0.0)) { *flags |= FLAG_MIX_ZERO; return 1.0f; }
    const double rms = sqrt(sm / (double)L) / 32768.0;
    double G = (double)lvl_amp / rms;
    if ((double)peak * G > 0.99) { G = 0.99 / (double)peak; *flags |= FLAG_LIMITED; }
    return (float)G;
}

__global__ __launch_bounds__(THREADS) void k_batch_plan(PlanArgs a, const unsigned long long* seed_step, Item* plan) {
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= a.B) return;
    plan[b] = plan_item(a, seed_step[0], seed_step[1], b);
}

// after the plan kernel in stream order: the next draw reads the next step
__global__ void k_batch_step(unsigned long long* seed_step) {
    if (blockIdx.x == 0 && threadIdx.x == 0) seed_step[1] = seed_step[1] + 1ull;
}

__device__ inline void store8(float* row, long i0, int cnt, bool vec, const float* y) {
    if (vec && cnt == GROUP) {
        float4* q = reinterpret_cast<float4*>(row + i0);
        q[0] = make_float4(y[0], y[1], y[2], y[3]);
        q[1] = make_float4(y[4], y[5], y[6], y[7]);
    } else {
#pragma unroll
        for (int k = 0; k < GROUP; ++k)
            if (k < cnt) row[i0 + k] = y[k];
    }
}

__global__ __launch_bounds__(THREADS) void k_batch_pairs(DrawArgs d, int tiles, bool vec) {
    const int b = blockIdx.x / tiles, t = blockIdx.x % tiles;
    const View v = view_of(d, b, true);
    const long i0 = (long)t * TILE + (long)threadIdx.x * GROUP;
    if (i0 >= d.L) return;
    const int cnt = d.L - i0 < GROUP ? (int)(d.L - i0) : GROUP;
    int x[GROUP], z[GROUP];
    load_clip8(v.s, v.len_s, v.sstart + i0, cnt, x);
    load_clip8(v.n, v.len_s, v.sstart + i0, cnt, z);
    float yx[GROUP], yz[GROUP];
#pragma unroll
    for (int k = 0; k < GROUP; ++k) {
        yx[k] = (float)x[k] * kScale;
        yz[k] = (float)z[k] * kScale;
    }
    store8(d.noisy + (long)b * d.noisy_stride, i0, cnt, vec, yx);
    store8(d.clean + (long)b * d.clean_stride, i0, cnt, vec, yz);
}

// pass 1: a chunk's three integer sums -> sums[b][c][0..2]
__global__ __launch_bounds__(THREADS) void k_batch_sums(DrawArgs d, int chunks, long ch) {
    __shared__ long long sm[THREADS / 64];
    const int b = blockIdx.x / chunks, c = blockIdx.x % chunks;
    const View v = view_of(d, b, false);
    const long lo = (long)c * ch, hi = lo + ch < d.L ? lo + ch : d.L;
    long long ss = 0, sn = 0, ssn = 0;
    for (long i0 = lo + (long)threadIdx.x * GROUP; i0 < hi; i0 += TILE) {
        const int cnt = hi - i0 < GROUP ? (int)(hi - i0) : GROUP;
        int x[GROUP], z[GROUP];
        load_clip8(v.s, v.len_s, v.sstart + i0, cnt, x);
        load_wrap8(v.n, v.len_n, wrap_index(v, i0), cnt, z);
#pragma unroll
        for (int k = 0; k < GROUP; ++k) {
            ss += (long long)(x[k] * x[k]);
            sn += (long long)(z[k] * z[k]);
            ssn += (long long)(x[k] * z[k]);
        }
    }
    ss = block_all<long long, false>(ss, sm);
    sn = block_all<long long, false>(sn, sm);
    ssn = block_all<long long, false>(ssn, sm);
    if (threadIdx.x == 0) {
        long long* out = d.sums + ((long)b * chunks + c) * 3;
        out[0] = ss; out[1] = sn; out[2] = ssn;
    }
}

// pass 2: the item's sums -> gn; a chunk's max |m_i| -> peaks[b][c]
__global__ __launch_bounds__(THREADS) void k_batch_peak(DrawArgs d, int chunks, long ch) {
    __shared__ long long sm[THREADS / 64];
    __shared__ float smf[THREADS / 64];
    const int b = blockIdx.x / chunks, c = blockIdx.x % chunks;
    const View v = view_of(d, b, false);
    const Sums s = item_sums(d.sums + (long)b * chunks * 3, chunks, sm);
    int flags = 0;
    const float gn = noise_gain(s, v.snr_amp, &flags);
    const long lo = (long)c * ch, hi = lo + ch < d.L ? lo + ch : d.L;
    float pk = 0.0f;
    for (long i0 = lo + (long)threadIdx.x * GROUP; i0 < hi; i0 += TILE) {
        const int cnt = hi - i0 < GROUP ? (int)(hi - i0) : GROUP;
        int x[GROUP], z[GROUP];
        load_clip8(v.s, v.len_s, v.sstart + i0, cnt, x);
        load_wrap8(v.n, v.len_n, wrap_index(v, i0), cnt, z);
#pragma unroll
        for (int k = 0; k < GROUP; ++k) {
            const float gz = gn * ((float)z[k] * kScale);
            const float m = (float)x[k] * kScale + gz;
            pk = fmaxf(pk, fabsf(m));
        }
    }
    pk = block_all<float, true>(pk, smf);
    if (threadIdx.x == 0) d.peaks[(long)b * chunks + c] = pk;
}

// pass 3: the item's sums and peak -> gn, Gf; the chunk's rows; chunk 0 writes the record
__global__ __launch_bounds__(THREADS) void k_batch_write(DrawArgs d, int chunks, long ch, bool vec) {
    __shared__ long long sm[THREADS / 64];
    __shared__ float smf[THREADS / 64];
    const int b = blockIdx.x / chunks, c = blockIdx.x % chunks;
    const View v = view_of(d, b, false);
    const Sums s = item_sums(d.sums + (long)b * chunks * 3, chunks, sm);
    const float peak = block_all<float, true>((int)threadIdx.x < chunks ? d.peaks[(long)b * chunks + threadIdx.x] : 0.0f, smf);
    int flags = 0;
    const float gn = noise_gain(s, v.snr_amp, &flags);
    const float Gf = level_gain(s, gn, peak, v.lvl_amp, d.L, &flags);
    if (c == 0 && threadIdx.x == 0) {
        Record r;
        r.Ss = s.ss; r.Sn = s.sn; r.Ssn = s.ssn;
        r.gn = gn; r.Gf = Gf; r.peak = peak; r.flags = flags;
        d.rec[b] = r;
    }
    float* noisy = d.noisy + (long)b * d.noisy_stride;
    float* clean = d.clean + (long)b * d.clean_stride;
    const long lo = (long)c * ch, hi = lo + ch < d.L ? lo + ch : d.L;
    for (long i0 = lo + (long)threadIdx.x * GROUP; i0 < hi; i0 += TILE) {
        const int cnt = hi - i0 < GROUP ? (int)(hi - i0) : GROUP;
        int x[GROUP], z[GROUP];
        load_clip8(v.s, v.len_s, v.sstart + i0, cnt, x);
        load_wrap8(v.n, v.len_n, wrap_index(v, i0), cnt, z);
        float yn[GROUP], yc[GROUP];
#pragma unroll
        for (int k = 0; k < GROUP; ++k) {
            const float sf = (float)x[k] * kScale;
            const float gz = gn * ((float)z[k] * kScale);
            const float m = sf + gz;
            yn[k] = Gf * m;
            yc[k] = Gf * sf;
        }
        store8(noisy, i0, cnt, vec, yn);
        store8(clean, i0, cnt, vec, yc);
    }
}

// pass 3 of the mix with a target: k_batch_write, but the clean row is the gained window of a target corpus that lies under
// the speech offsets table (three 16-byte loads and four 16-byte stores per 8 samples).  Sums, gains, peak, record and noisy
// are the speech side's: with target == the speech corpus this writes what k_batch_write writes, bit for bit.
__global__ __launch_bounds__(THREADS) void k_batch_write_target(DrawArgs d, const short* target, int chunks, long ch, bool vec) {
    __shared__ long long sm[THREADS / 64];
    __shared__ float smf[THREADS / 64];
    const int b = blockIdx.x / chunks, c = blockIdx.x % chunks;
    const View v = view_of(d, b, false);
    const short* tg = target + (v.s - d.a.pcm);        // the same clip of the parallel corpus
    const Sums s = item_sums(d.sums + (long)b * chunks * 3, chunks, sm);
    const float peak = block_all<float, true>((int)threadIdx.x < chunks ? d.peaks[(long)b * chunks + threadIdx.x] : 0.0f, smf);
    int flags = 0;
    const float gn = noise_gain(s, v.snr_amp, &flags);
    const float Gf = level_gain(s, gn, peak, v.lvl_amp, d.L, &flags);
    if (c == 0 && threadIdx.x == 0) {
        Record r;
        r.Ss = s.ss; r.Sn = s.sn; r.Ssn = s.ssn;
        r.gn = gn; r.Gf = Gf; r.peak = peak; r.flags = flags;
        d.rec[b] = r;
    }
    float* noisy = d.noisy + (long)b * d.noisy_stride;
    float* clean = d.clean + (long)b * d.clean_stride;
    const long lo = (long)c * ch, hi = lo + ch < d.L ? lo + ch : d.L;
    for (long i0 = lo + (long)threadIdx.x * GROUP; i0 < hi; i0 += TILE) {
        const int cnt = hi - i0 < GROUP ? (int)(hi - i0) : GROUP;
        int x[GROUP], z[GROUP], t[GROUP];
        load_clip8(v.s, v.len_s, v.sstart + i0, cnt, x);
        load_wrap8(v.n, v.len_n, wrap_index(v, i0), cnt, z);
        load_clip8(tg, v.len_s, v.sstart + i0, cnt, t);
        float yn[GROUP], yc[GROUP];
#pragma unroll
        for (int k = 0; k < GROUP; ++k) {
            const float sf = (float)x[k] * kScale;
            const float gz = gn * ((float)z[k] * kScale);
            const float m = sf + gz;
            yn[k] = Gf * m;
            yc[k] = Gf * ((float)t[k] * kScale);
        }
        store8(noisy, i0, cnt, vec, yn);
        store8(clean, i0, cnt, vec, yc);
    }
}

// ---- active levels: the mix at an SNR of the levels over active windows ("active levels" in the header) ----
// A row is judged in windows of W samples (a multiple of GROUP, so a thread's 16-byte group never straddles a window); a chunk
// is a whole number of windows (batch.h).  A window's energy is an exact 64-bit integer and its activity an integer
// comparison, so the four active sums are as order-free as the three plain ones.

// N sums of a workgroup at once, returned to every thread.  sm: (THREADS / 64) * N values.
template <int N>
__device__ inline void block_sums(long long* v, long long* sm) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[j] += __shfl_xor(v[j], o, 64);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j) sm[(threadIdx.x >> 6) * N + j] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) {
        long long r = sm[j];
#pragma unroll
        for (int k = 1; k < THREADS / 64; ++k) r += sm[k * N + j];
        v[j] = r;
    }
}

struct ActiveSums {
    Sums s;                    // the whole row's, as in the plain mix
    long long As, An;          // energy over the active windows of each side
    long long Ns, Nn;          // samples in them (at most L)
};

// an item's seven sums from its chunks' partials (chunks <= THREADS)
__device__ inline ActiveSums active_item_sums(const long long* part, int chunks, long long* sm) {
    long long p[ACTIVE_PARTS];
#pragma unroll
    for (int j = 0; j < ACTIVE_PARTS; ++j) p[j] = (int)threadIdx.x < chunks ? part[ACTIVE_PARTS * threadIdx.x + j] : 0;
    block_sums<ACTIVE_PARTS>(p, sm);
    ActiveSums a;
    a.s.ss = p[0]; a.s.sn = p[1]; a.s.ssn = p[2];
    a.As = p[3]; a.Ns = p[4]; a.An = p[5]; a.Nn = p[6];
    return a;
}

// The fallback (a side without an active window is levelled over the whole row), then gn in the contract's operation order.
__device__ inline float noise_gain_active(ActiveSums* a, float snr_amp, long L, int* flags) {
    if (a->Ns == 0) { a->As = a->s.ss; a->Ns = L; *flags |= FLAG_SPEECH_INACTIVE; }
    if (a->Nn == 0) { a->An = a->s.sn; a->Nn = L; *flags |= FLAG_NOISE_INACTIVE; }
    if (a->An == 0) { *flags |= FLAG_NOISE_ZERO; return 0.0f; }
    if (a->As == 0) { *flags |= FLAG_SPEECH_ZERO; return 1.0f; }
    double r = (double)a->As / (double)a->An;
    if (a->Ns != a->Nn) r = r * ((double)a->Nn / (double)a->Ns);
    return (float)(sqrt(r) * (double)snr_amp);
}

// a value every lane of the wave holds, moved into scalar registers: what is added up per window then costs no vector register
__device__ inline long long wave_uniform(long long v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// pass 1: one wave per window.  Its lanes stride the window's groups, both energies are reduced across the wave and every
// lane then holds the window's two decisions; the chunk's seven partials -> sums[b][c][0..6]
__global__ __launch_bounds__(THREADS) void k_batch_active_sums(DrawArgs d, int W, long long thr, int chunks, long ch) {
    __shared__ long long sm[(THREADS / 64) * ACTIVE_PARTS];
    const int b = blockIdx.x / chunks, c = blockIdx.x % chunks;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const View v = view_of(d, b, false);
    const long lo = (long)c * ch, hi = lo + ch < d.L ? lo + ch : d.L;
    long long ss = 0, sn = 0, ssn = 0, as = 0, ns = 0, an = 0, nn = 0;      // ssn per lane, the others per wave
#pragma unroll 1
    for (long w0 = lo + (long)wave * W; w0 < hi; w0 += (long)(THREADS / 64) * W) {
        const long w1 = w0 + W < hi ? w0 + W : hi;
        long long es = 0, en = 0;
        // A window of whole groups that lies inside the speech clip and does not wrap the noise (all but a few of a batch):
        // four 16-byte loads per side and lane are in flight at once, a lane past the window's end reads its last group and
        // counts zeros.  Any other window goes group by group through the checked loads.
        const unsigned j0 = wrap_index(v, w0);
        const int ng = (int)((w1 - w0) / GROUP);
        const bool inside = (w1 - w0) % GROUP == 0 && v.sstart + w1 <= v.len_s && (unsigned long long)j0 + (unsigned long long)(w1 - w0) <= v.len_n;
        const short* ps = v.s + (v.sstart + w0);
        const short* pn = v.n + j0;
#pragma unroll 1
        for (int g0 = lane; inside && g0 - lane < ng; g0 += 4 * 64) {
            short ts[4][GROUP], tn[4][GROUP];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int g = g0 + 64 * u < ng ? g0 + 64 * u : ng - 1;
                __builtin_memcpy(ts[u], ps + (long)g * GROUP, sizeof(ts[u]));
                __builtin_memcpy(tn[u], pn + (long)g * GROUP, sizeof(tn[u]));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool on = g0 + 64 * u < ng;
#pragma unroll
                for (int k = 0; k < GROUP; ++k) {
                    const int x = on ? (int)ts[u][k] : 0, z = on ? (int)tn[u][k] : 0;
                    es += (long long)(x * x);
                    en += (long long)(z * z);
                    ssn += (long long)(x * z);
                }
            }
        }
#pragma unroll 1
        for (long i0 = w0 + (long)lane * GROUP; !inside && i0 < w1; i0 += 64 * GROUP) {
            const int cnt = w1 - i0 < GROUP ? (int)(w1 - i0) : GROUP;
            int x[GROUP], z[GROUP];
            load_clip8(v.s, v.len_s, v.sstart + i0, cnt, x);
            load_wrap8(v.n, v.len_n, wrap_index(v, i0), cnt, z);
#pragma unroll
            for (int k = 0; k < GROUP; ++k) {
                es += (long long)(x[k] * x[k]);
                en += (long long)(z[k] * z[k]);
                ssn += (long long)(x[k] * z[k]);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            es += __shfl_xor(es, o, 64);
            en += __shfl_xor(en, o, 64);
        }
        es = wave_uniform(es);
        en = wave_uniform(en);
        const long long bar = thr * (long long)(w1 - w0);
        ss += es;
        sn += en;
        if (es > bar) { as += es; ns += w1 - w0; }
        if (en > bar) { an += en; nn += w1 - w0; }
    }
    const bool first = lane == 0;
    long long p[ACTIVE_PARTS] = {first ? ss : 0, first ? sn : 0, ssn, first ? as : 0, first ? ns : 0, first ? an : 0, first ? nn : 0};
    block_sums<ACTIVE_PARTS>(p, sm);
    if (threadIdx.x == 0) {
        long long* out = d.sums + ((long)b * chunks + c) * ACTIVE_PARTS;
#pragma unroll
        for (int j = 0; j < ACTIVE_PARTS; ++j) out[j] = p[j];
    }
}

// pass 2: k_batch_peak with the item's seven sums and the active gain
__global__ __launch_bounds__(THREADS) void k_batch_active_peak(DrawArgs d, int chunks, long ch) {
    __shared__ long long sm[(THREADS / 64) * ACTIVE_PARTS];
    __shared__ float smf[THREADS / 64];
    const int b = blockIdx.x / chunks, c = blockIdx.x % chunks;
    const View v = view_of(d, b, false);
    ActiveSums a = active_item_sums(d.sums + (long)b * chunks * ACTIVE_PARTS, chunks, sm);
    int flags = 0;
    const float gn = noise_gain_active(&a, v.snr_amp, d.L, &flags);
    const long lo = (long)c * ch, hi = lo + ch < d.L ? lo + ch : d.L;
    float pk = 0.0f;
    for (long i0 = lo + (long)threadIdx.x * GROUP; i0 < hi; i0 += TILE) {
        const int cnt = hi - i0 < GROUP ? (int)(hi - i0) : GROUP;
        int x[GROUP], z[GROUP];
        load_clip8(v.s, v.len_s, v.sstart + i0, cnt, x);
        load_wrap8(v.n, v.len_n, wrap_index(v, i0), cnt, z);
#pragma unroll
        for (int k = 0; k < GROUP; ++k) {
            const float gz = gn * ((float)z[k] * kScale);
            const float m = (float)x[k] * kScale + gz;
            pk = fmaxf(pk, fabsf(m));
        }
    }
    pk = block_all<float, true>(pk, smf);
    if (threadIdx.x == 0) d.peaks[(long)b * chunks + c] = pk;
}

// pass 3: k_batch_write (TARGET: k_batch_write_target; `target` is not read otherwise) with the item's seven sums, the active
// gain and the 64-byte record
template <bool TARGET>
__global__ __launch_bounds__(THREADS) void k_batch_active_write(DrawArgs d, const short* target, ActiveRecord* rec, int chunks, long ch,
                                                                bool vec) {
    __shared__ long long sm[(THREADS / 64) * ACTIVE_PARTS];
    __shared__ float smf[THREADS / 64];
    const int b = blockIdx.x / chunks, c = blockIdx.x % chunks;
    const View v = view_of(d, b, false);
    const short* tg = TARGET ? target + (v.s - d.a.pcm) : v.s;          // the same clip of the parallel corpus
    ActiveSums a = active_item_sums(d.sums + (long)b * chunks * ACTIVE_PARTS, chunks, sm);
    const float peak = block_all<float, true>((int)threadIdx.x < chunks ? d.peaks[(long)b * chunks + threadIdx.x] : 0.0f, smf);
    int flags = 0;
    const float gn = noise_gain_active(&a, v.snr_amp, d.L, &flags);
    const float Gf = level_gain(a.s, gn, peak, v.lvl_amp, d.L, &flags);
    if (c == 0 && threadIdx.x == 0) {
        ActiveRecord r;
        r.Ss = a.s.ss; r.Sn = a.s.sn; r.Ssn = a.s.ssn; r.As = a.As; r.An = a.An;
        r.Ns = (int)a.Ns; r.Nn = (int)a.Nn;
        r.gn = gn; r.Gf = Gf; r.peak = peak; r.flags = flags;
        rec[b] = r;
    }
    float* noisy = d.noisy + (long)b * d.noisy_stride;
    float* clean = d.clean + (long)b * d.clean_stride;
    const long lo = (long)c * ch, hi = lo + ch < d.L ? lo + ch : d.L;
    for (long i0 = lo + (long)threadIdx.x * GROUP; i0 < hi; i0 += TILE) {
        const int cnt = hi - i0 < GROUP ? (int)(hi - i0) : GROUP;
        int x[GROUP], z[GROUP], t[GROUP];
        load_clip8(v.s, v.len_s, v.sstart + i0, cnt, x);
        load_wrap8(v.n, v.len_n, wrap_index(v, i0), cnt, z);
        if (TARGET) load_clip8(tg, v.len_s, v.sstart + i0, cnt, t);
        float yn[GROUP], yc[GROUP];
#pragma unroll
        for (int k = 0; k < GROUP; ++k) {
            const float sf = (float)x[k] * kScale;
            const float gz = gn * ((float)z[k] * kScale);
            const float m = sf + gz;
            yn[k] = Gf * m;
            yc[k] = Gf * (TARGET ? (float)t[k] * kScale : sf);
        }
        store8(noisy, i0, cnt, vec, yn);
        store8(clean, i0, cnt, vec, yc);
    }
}

bool rows_take_16_bytes(const DrawArgs& d) {
    return (reinterpret_cast<uintptr_t>(d.noisy) & 15) == 0 && (reinterpret_cast<uintptr_t>(d.clean) & 15) == 0 &&
           d.noisy_stride % 4 == 0 && d.clean_stride % 4 == 0;
}

}  // namespace

int launch_plan(const PlanArgs& a, unsigned long long* d_seed_step, int advance, Item* d_plan, hipStream_t s) {
    hipLaunchKernelGGL(k_batch_plan, dim3((a.B + THREADS - 1) / THREADS), dim3(THREADS), 0, s, a, d_seed_step, d_plan);
    if (advance) hipLaunchKernelGGL(k_batch_step, dim3(1), dim3(64), 0, s, d_seed_step);
    return (int)hipGetLastError();
}

int launch_pairs(const DrawArgs& d, hipStream_t s) {
    const int tiles = (int)((d.L + TILE - 1) / TILE);
    hipLaunchKernelGGL(k_batch_pairs, dim3((unsigned)((long)d.B * tiles)), dim3(THREADS), 0, s, d, tiles, rows_take_16_bytes(d));
    return (int)hipGetLastError();
}

int launch_mix(const DrawArgs& d, int passes, hipStream_t s) {
    const int chunks = chunks_of(d.L);
    const long ch = chunk_samples(d.L);
    const dim3 grid((unsigned)((long)d.B * chunks)), block(THREADS);
    if (passes & 1) hipLaunchKernelGGL(k_batch_sums, grid, block, 0, s, d, chunks, ch);
    if (passes & 2) hipLaunchKernelGGL(k_batch_peak, grid, block, 0, s, d, chunks, ch);
    if (passes & 4) hipLaunchKernelGGL(k_batch_write, grid, block, 0, s, d, chunks, ch, rows_take_16_bytes(d));
    return (int)hipGetLastError();
}

int launch_mix_target(const DrawArgs& d, const short* d_target, int passes, hipStream_t s) {
    const int chunks = chunks_of(d.L);
    const long ch = chunk_samples(d.L);
    const dim3 grid((unsigned)((long)d.B * chunks)), block(THREADS);
    if (passes & 1) hipLaunchKernelGGL(k_batch_sums, grid, block, 0, s, d, chunks, ch);
    if (passes & 2) hipLaunchKernelGGL(k_batch_peak, grid, block, 0, s, d, chunks, ch);
    if (passes & 4) hipLaunchKernelGGL(k_batch_write_target, grid, block, 0, s, d, d_target, chunks, ch, rows_take_16_bytes(d));
    return (int)hipGetLastError();
}

int launch_mix_active(const DrawArgs& d, const short* d_target, ActiveRecord* rec, int W, long long thr, int passes, hipStream_t s) {
    const int chunks = active_chunks_of(d.L, W);
    const long ch = active_chunk_samples(d.L, W);
    const dim3 grid((unsigned)((long)d.B * chunks)), block(THREADS);
    const bool vec = rows_take_16_bytes(d);
    if (passes & 1) hipLaunchKernelGGL(k_batch_active_sums, grid, block, 0, s, d, W, thr, chunks, ch);
    if (passes & 2) hipLaunchKernelGGL(k_batch_active_peak, grid, block, 0, s, d, chunks, ch);
    if (passes & 4) {
        if (d_target) hipLaunchKernelGGL(k_batch_active_write<true>, grid, block, 0, s, d, d_target, rec, chunks, ch, vec);
        else hipLaunchKernelGGL(k_batch_active_write<false>, grid, block, 0, s, d, d_target, rec, chunks, ch, vec);
    }
    return (int)hipGetLastError();
}

}  // namespace gtb
