// batch.h -- training batches from a resident corpus ("training batches from a resident corpus" in
// include/gtcrn_micro_hip.h): the plan's arithmetic as one __host__ __device__ body (batch.hip runs it per item on the
// device, batch_host.cpp on the host for gtcrn_batch_plan_host) and the launch interface of batch.hip.
// Both files are compiled with -ffp-contract=off: the contract is stated operation by operation.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace gtb {

struct Item {                          // == gtcrn_batch_item, 32 bytes
    int sclip, sstart, nclip, nstart;
    float snr_db, snr_amp, lvl_db, lvl_amp;
};

struct Record {                        // == gtcrn_batch_record, 40 bytes
    long long Ss, Sn, Ssn;
    float gn, Gf, peak;
    int flags;
};

struct ActiveRecord {                  // == gtcrn_batch_active_record, 64 bytes; As, An, Ns, Nn as used (after the fallback)
    long long Ss, Sn, Ssn, As, An;
    int Ns, Nn;
    float gn, Gf, peak;
    int flags;
};

enum { FLAG_NOISE_ZERO = 1, FLAG_SPEECH_ZERO = 2, FLAG_MIX_ZERO = 4, FLAG_LIMITED = 8, FLAG_SPEECH_INACTIVE = 16,
       FLAG_NOISE_INACTIVE = 32 };

constexpr int THREADS = 256;           // four waves
constexpr int GROUP = 8;               // samples a thread handles at a time: 16 bytes in, 2 x 16 bytes out
constexpr int TILE = THREADS * GROUP;  // samples one pass of a workgroup covers
constexpr int MAX_CHUNKS = 256;        // an item's partials are added up by one workgroup pass, one per thread
constexpr long MAX_L = (1L << 31) - 1;

// Samples per workgroup of the mix passes: two tiles, or what keeps an item within MAX_CHUNKS chunks.
__host__ __device__ inline long chunk_samples(long L) {
    long ch = 2 * TILE;
    const long need = (L + MAX_CHUNKS - 1) / MAX_CHUNKS;
    if (need > ch) ch = (need + TILE - 1) / TILE * TILE;
    return ch;
}
__host__ __device__ inline int chunks_of(long L) { return (int)((L + chunk_samples(L) - 1) / chunk_samples(L)); }

// "active levels": the same cut for a row that is judged in windows of W samples (a multiple of GROUP).  A chunk is a whole
// number of windows: as few as cover two tiles, or what keeps an item within MAX_CHUNKS chunks.  W = 1600: 3 windows, 4800 samples.
constexpr int MIN_WINDOW = GROUP, MAX_WINDOW = 1 << 20;
constexpr long long MAX_THRESHOLD = 1LL << 30;
constexpr int ACTIVE_PARTS = 7;        // a chunk's partials: Ss, Sn, Ssn, As, Ns, An, Nn
__host__ __device__ inline long active_chunk_windows(long L, int W) {
    long k = (2 * TILE + W - 1) / W;
    const long windows = (L + W - 1) / W;
    const long need = (windows + MAX_CHUNKS - 1) / MAX_CHUNKS;
    return need > k ? need : k;
}
__host__ __device__ inline long active_chunk_samples(long L, int W) { return active_chunk_windows(L, W) * W; }
__host__ __device__ inline int active_chunks_of(long L, int W) {
    return (int)((L + active_chunk_samples(L, W) - 1) / active_chunk_samples(L, W));
}

struct PlanArgs {
    const long long* soff = nullptr;   // [n_speech + 1]
    const long long* noff = nullptr;   // [n_noise + 1], or null (pairs: nclip = nstart = 0)
    int n_speech = 0, n_noise = 0;
    int B = 0;
    long L = 0, item0 = 0;
    int granule = 1;
    float snr_lo = 0, snr_hi = 0, lvl_lo = 0, lvl_hi = 0;
    const int* clips = nullptr;        // [B] or null
};

__host__ __device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t* out) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__host__ __device__ inline uint32_t mulhi32(uint32_t r, uint32_t k) { return (uint32_t)(((uint64_t)r * k) >> 32); }
__host__ __device__ inline float unit24(uint32_t q) { return (float)(q >> 8) * 5.9604644775390625e-08f; }   // 2^-24, exact
__host__ __device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// Item b of a plan: a pure function of (seed, step, item0 + b) and the tables.
__host__ __device__ inline Item plan_item(const PlanArgs& a, uint64_t seed, uint64_t step, int b) {
    uint32_t r[4], q[4];
    const uint32_t c0 = (uint32_t)((uint64_t)a.item0 + (uint64_t)b);
    philox4x32_10(c0, (uint32_t)step, (uint32_t)(step >> 32), 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    philox4x32_10(c0, (uint32_t)step, (uint32_t)(step >> 32), 1u, (uint32_t)seed, (uint32_t)(seed >> 32), q);
    Item it;
    // a clip id of the caller's outside the table is a broken precondition; it is clamped so that nothing reads out of bounds
    it.sclip = a.clips ? clampi(a.clips[b], 0, a.n_speech - 1) : (int)mulhi32(r[0], (uint32_t)a.n_speech);
    const long long len_s = a.soff[it.sclip + 1] - a.soff[it.sclip];
    long long ks = len_s < a.L ? 1 : (len_s - a.L) / a.granule + 1;
    if (ks < 1) ks = 1;
    it.sstart = (int)((long long)a.granule * (long long)mulhi32(r[1], (uint32_t)ks));
    it.nclip = 0;
    it.nstart = 0;
    if (a.noff) {
        it.nclip = (int)mulhi32(r[2], (uint32_t)a.n_noise);
        const long long len_n = a.noff[it.nclip + 1] - a.noff[it.nclip];
        it.nstart = (int)mulhi32(r[3], (uint32_t)(len_n > 0 ? len_n : 0));
    }
    it.snr_db = a.snr_lo + (a.snr_hi - a.snr_lo) * unit24(q[0]);
    it.lvl_db = a.lvl_lo + (a.lvl_hi - a.lvl_lo) * unit24(q[1]);
    it.snr_amp = (float)pow(10.0, -(double)it.snr_db / 20.0);
    it.lvl_amp = (float)pow(10.0, (double)it.lvl_db / 20.0);
    return it;
}

struct Corpus {
    const short* pcm = nullptr;
    const long long* off = nullptr;
    int n = 0;
};

struct DrawArgs {
    Corpus a, b;                       // mix: speech, noise; pairs: noisy, clean (one offsets table)
    const Item* plan = nullptr;
    int B = 0;
    long L = 0;
    float* noisy = nullptr;
    float* clean = nullptr;
    long noisy_stride = 0, clean_stride = 0;
    Record* rec = nullptr;             // mix only
    long long* sums = nullptr;         // mix only: [B][chunks][3]
    float* peaks = nullptr;            // mix only: [B][chunks]
};

// Every launch_* returns 0 or a hipError_t.
int launch_plan(const PlanArgs& a, unsigned long long* d_seed_step, int advance, Item* d_plan, hipStream_t s);
int launch_pairs(const DrawArgs& d, hipStream_t s);
// The three launches of a mix draw, in stream order: passes = 7; a subset (1 sums, 2 peak, 4 write) launches only those.
int launch_mix(const DrawArgs& d, int passes, hipStream_t s);
// The same with the clean rows cut from d_target, a corpus under the speech offsets table: passes 1 and 2 are launch_mix's
// kernels, pass 3 is a write kernel of its own.
int launch_mix_target(const DrawArgs& d, const short* d_target, int passes, hipStream_t s);
// The mix at an SNR of active levels ("active levels"): three kernels of its own over the active_* geometry.  d.sums holds
// [B][chunks][ACTIVE_PARTS], d.rec is not used (the records are `rec`), d_target may be null (clean is cut from the speech).
int launch_mix_active(const DrawArgs& d, const short* d_target, ActiveRecord* rec, int W, long long thr, int passes, hipStream_t s);

}  // namespace gtb
