// reverb.h -- reverberant speech for resident-corpus batches ("reverberant speech: exact RIR convolution" in
// include/gtcrn_micro_hip.h): the reverb plan's arithmetic as one __host__ __device__ body
// (reverb.hip runs it per row on the device, reverb_host.cpp on the host), the digit scheme and the table geometry both
// files share, and the launch interface of reverb.hip; behind them the geometry of the split table and the launch interface
// of the split convolution ("dereverberation targets: early or direct clean").
#pragma once
#include "batch.h"

namespace gtr {

struct RItem { int rir, reserved; };                       // == gtcrn_reverb_item, 8 bytes
struct RRecord { int rir, ntaps, saturated, reserved; };   // == gtcrn_reverb_record, 16 bytes

constexpr int MAX_TAPS = 16384;        // 1.024 s at 16 kHz
constexpr int TAP_MAX = 32639;         // |tap| bound of a bank: 127 * 256 + 127, so both balanced digits fit int8
constexpr int THREADS = 256;           // four waves
constexpr int BLOCK = 2048;            // output samples of one workgroup: 8 rows of 64000 already give 256 workgroups
constexpr int BIG_BLOCK = 8192;        // ... of the matrix form once blocks of this size fill the machine as well
constexpr int FILL = 256;              // workgroups that fill the machine (one per compute unit)
constexpr int GROUP_BYTES = 512;       // one 16-tap group of the derived table: a 16 x 16 int8 tile per digit, hi then lo
constexpr int MAX_GROUPS = 16 * ((MAX_TAPS + 15 + 255) / 256);

// Taps of a response by its offsets; a length outside 1 .. MAX_TAPS is a broken table and counts as no response.
__host__ __device__ inline int taps_of(long long len) { return len < 1 || len > MAX_TAPS ? 0 : (int)len; }
// 16-wide groups of u = 0 .. K + 14 (u = k - j + 15 for tap k and output j of a 16-group): whole 64-chunks, and of those
// whole fours (the matrix form's loop body is four chunks; the padding is zero taps)
__host__ __device__ inline int groups_of(int K) { return 16 * ((K + 15 + 255) / 256); }
// Output samples per workgroup of the matrix form: form 2 takes the large block when B rows of it fill the machine, forms 3
// and 4 pin the small and the large one (the A/B switch of tests and measurements).
inline long block_of(int form, int B, long L) {
    if (form == 3) return BLOCK;
    if (form == 4) return BIG_BLOCK;
    return (long long)B * ((L + BIG_BLOCK - 1) / BIG_BLOCK) >= FILL ? BIG_BLOCK : BLOCK;
}
__host__ __device__ inline long long header_bytes(int n) { return ((long long)n * 16 + 255) & ~255LL; }

// The digits.  A tap h in -TAP_MAX .. TAP_MAX is 256 * tap_hi + tap_lo with both in -127 .. 127 (balanced).  A speech
// sample x, ANY int16, is 256 * (x >> 8) + speech_lo(x) + 128 with speech_lo = (x & 255) - 128: both in -128 .. 127, and
// zero padding is stored as the digits of 0, so the + 128 belongs to every term and sums to 128 * sum(h).
__host__ __device__ inline int tap_lo(int h) { return ((h + 128) & 255) - 128; }
__host__ __device__ inline int tap_hi(int h) { return (h - tap_lo(h)) >> 8; }

// Row b of a reverb plan: Philox block k = 2 of the batch plan's counter and key.
__host__ __device__ inline RItem reverb_item(int n_rir, float p_reverb, long item0, uint64_t seed, uint64_t step, int b) {
    uint32_t t[4];
    const uint32_t c0 = (uint32_t)((uint64_t)item0 + (uint64_t)b);
    gtb::philox4x32_10(c0, (uint32_t)step, (uint32_t)(step >> 32), 2u, (uint32_t)seed, (uint32_t)(seed >> 32), t);
    RItem it;
    it.rir = gtb::unit24(t[0]) < p_reverb ? (int)gtb::mulhi32(t[1], (uint32_t)n_rir) : -1;
    it.reserved = 0;
    return it;
}

struct ReverbArgs {
    gtb::Corpus speech;
    const short* taps = nullptr;
    const long long* roff = nullptr;           // [n_rir + 1]
    int n_rir = 0;
    const unsigned char* table = nullptr;      // matrix form only
    long long table_bytes = 0;
    const gtb::Item* plan = nullptr;
    const RItem* rplan = nullptr;
    int B = 0;
    long L = 0;
    short* staged = nullptr;                   // [B][stride]
    long stride = 0;
    long long* soffsets = nullptr;             // [B + 1]
    gtb::Item* splan = nullptr;                // [B]
    RRecord* rec = nullptr;                    // [B]
    int* partial = nullptr;                    // [B][blocks]: clamped samples of each workgroup
    int blocks = 0;
};

// ---- the split convolution ("dereverberation targets: early or direct clean" in the header) ----------
struct SRecord { int rir, ntaps, saturated, split, target_saturated, r0, r1, r2; };   // == gtcrn_reverb_split_record, 32 bytes

// Split of a response of K taps (K >= 1): any value is clamped into 1 .. K.
__host__ __device__ inline int split_of(int e, int K) { return e < 1 ? 1 : e > K ? K : e; }
// The split table of a response: its early segment, taps 0 .. E - 1 in the tile format above (groups_of(E) groups), then its
// rest segment, groups rest_first(E) .. groups_of(K) - 1 of the response with the taps below E stored as zero -- absent when
// E == K.  Both are whole fours of 64-tap chunks, and they are contiguous.
__host__ __device__ inline int rest_first(int E) { return 16 * (E / 256); }
__host__ __device__ inline int rest_groups(int E, int K) { return E >= K ? 0 : groups_of(K) - rest_first(E); }
// header: per response {int64 byte offset of its groups, int64 sum of its taps below E, int64 sum of its taps, int64 E}
__host__ __device__ inline long long split_header_bytes(int n) { return ((long long)n * 32 + 255) & ~255LL; }

struct SplitArgs {
    ReverbArgs r;                              // r.staged: the wet rows; r.rec is not used; r.partial: [2][B][blocks]
    const int* split = nullptr;                // [n_rir]
    short* target = nullptr;                   // [B][r.stride]
    SRecord* srec = nullptr;                   // [B]
};

// Every launch_* returns 0 or a hipError_t.
int launch_split_prepare(const short* d_taps, const long long* d_roff, const int* d_split, int n_rir, unsigned char* d_table,
                         long long table_bytes, hipStream_t s);
int launch_split(SplitArgs a, int form, hipStream_t s);     // forms as launch_reverb; sets a.r.blocks
int launch_reverb_plan(int n_rir, float p_reverb, int B, long item0, const unsigned long long* d_seed_step, RItem* d_rplan,
                       hipStream_t s);
int launch_reverb_prepare(const short* d_taps, const long long* d_roff, int n_rir, unsigned char* d_table, long long table_bytes,
                          hipStream_t s);
int launch_reverb(ReverbArgs a, int form, hipStream_t s);   // form 1 plain, 2 matrix, 3 / 4 matrix with the block pinned; sets a.blocks
int launch_selftest_i8(const signed char* dA, const signed char* dB, const int* dC, int* dD, hipStream_t s);

}  // namespace gtr
