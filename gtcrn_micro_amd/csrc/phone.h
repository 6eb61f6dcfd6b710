// phone.h -- telephone-channel rows for resident-corpus batches ("telephone-channel rows: exact 8 kHz band + G.711" in
// include/gtcrn_micro_hip.h): the filter table, the phone plan's arithmetic and steps 1 - 5 of the
// channel as one set of __host__ __device__ functions (phone.hip runs them per workgroup on the device, phone_host.cpp per
// row on the host for gtcrn_batch_phone_host), the chunk geometry both files share and the launch interface of phone.hip.
// Both files are compiled with -ffp-contract=off like the batch and reverb files; but for step 1's one rounded multiply
// and the plan's one float compare everything here is integer arithmetic.
#pragma once
#include "batch.h"
#include "kernels.h"   // gtk::g711_encode / gtk::g711_decode: the one statement of both laws ("G.711 payloads")

namespace gtp {

struct PItem { int codec, reserved; };                              // == gtcrn_phone_item, 8 bytes
struct PRecord { int codec, saturated_down, saturated_up, reserved; };   // == gtcrn_phone_record, 16 bytes

constexpr int NTAPS = 129, HALF = 64;

// T[0 .. 64] of the table (T[k] == T[128 - k]): rint(32768 h[n]) of the 16 kHz -> 8 kHz design of "sample-rate conversion".
// A literal, so that every tap of the unrolled loops below is a constant of the instruction stream (and a zero tap no
// instruction at all).  design_taps (phone_host.cpp) designs the table again in double, and gtcrn_batch_phone_taps refuses
// to return a table that differs from this one in a single entry.
constexpr short TAPS_HALF[HALF + 1] = {
    0, 0, 0, 1, 0, -1, -1, 2, 2, -2, -4, 2, 6, -2, -9, 1, 13, 1, -18, -6, 22, 13, -27, -23, 29, 36, -30, -53, 26, 73, -17, -94, 0,
    117, 25, -138, -61, 155, 108, -165, -166, 164, 236, -147, -316, 109, 404, -44, -499, -54, 596, 195, -691, -394, 782, 676,
    -863, -1095, 931, 1793, -982, -3296, 1013, 10370, 15360};
// T[k]; 0 outside 0 .. 128 (the pairs below reach one tap past either end)
__host__ __device__ constexpr int tap(int k) { return k < 0 || k > 2 * HALF ? 0 : TAPS_HALF[k <= HALF ? k : 2 * HALF - k]; }

// sum of |T[k]| over k = lo .. hi in steps of `step`
constexpr long long abs_taps(int lo, int hi, int step) {
    long long s = 0;
    for (int k = lo; k <= hi; k += step) s += tap(k) < 0 ? -tap(k) : tap(k);
    return s;
}
// The accumulators.  A sum over all 129 taps reaches 69558 * 32768 = 2.28e9 and does not fit 32 bits, so no 32-bit
// accumulator below ever holds one: the decimator adds taps 65 .. 128 and taps 0 .. 64 into two int32 partial sums and joins
// them in 64 bits; the interpolator's two polyphase halves (the even taps for an even output, the odd taps for an odd one) are
// one int32 each.  Every operand is an int16 (|x| <= 32768), so each partial sum is bounded by 32768 * sum |T| of its taps:
static_assert(abs_taps(0, 128, 1) == 69558, "the table of the contract");
static_assert(32768 * abs_taps(65, 128, 1) < (1LL << 31) && 32768 * abs_taps(0, 64, 1) < (1LL << 31), "decimator halves fit int32");
static_assert(32768 * abs_taps(0, 128, 2) < (1LL << 31) && 32768 * abs_taps(1, 127, 2) < (1LL << 31), "polyphase halves fit int32");

// Two int16 as the pair the dot products take: `lo` is the lower-indexed sample.
__host__ __device__ constexpr uint32_t pack2(int lo, int hi) { return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16); }
// c + a.lo * b.lo + a.hi * b.hi on int16 halves, in int32 (v_dot2_i32_i16 on the device).  The callers keep |result| < 2^31.
__host__ __device__ inline int dot2(uint32_t a, uint32_t b, int c) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short v2s __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, a), __builtin_bit_cast(v2s, b), c, false);
#else
    return c + (int)(short)(a & 0xFFFFu) * (int)(short)(b & 0xFFFFu) + (int)(short)(a >> 16) * (int)(short)(b >> 16);
#endif
}

// ---- steps 1 - 5 ------------------------------------------------------------------------------------------------------------
// Step 1: clip(rint(32768 r), -32768, 32767), half to even.  The product is exact (a power of two) unless it overflows, and
// then the clip takes it.  A NaN becomes -32768: unspecified audio, but an int16 like any other, on the host and the device.
__host__ __device__ inline int pcm_of(float r) {
    float x = 32768.0f * r;
    x = x >= -32768.0f ? x : -32768.0f;
    x = x <= 32767.0f ? x : 32767.0f;
    return (int)rintf(x);
}
__host__ __device__ inline int sat16(long long v, int* clips) {
    if (v < -32768) { ++*clips; return -32768; }
    if (v > 32767) { ++*clips; return 32767; }
    return (int)v;
}
// Step 2 for one j.  q[m] = pack2(p[2j - 64 + 2m], p[2j - 63 + 2m]), m = 0 .. 64: the sample n = 2m (+1) of that window meets
// tap 128 - n; the odd half of the last pair meets no tap.
__host__ __device__ inline int decimate_at(const uint32_t* q, int* clips) {
    int far = 0, near = 0;                             // taps 128 .. 65, taps 64 .. 0
#pragma unroll
    for (int m = 0; m < 32; ++m) far = dot2(q[m], pack2(tap(128 - 2 * m), tap(127 - 2 * m)), far);
#pragma unroll
    for (int m = 32; m < 65; ++m) near = dot2(q[m], pack2(tap(128 - 2 * m), tap(127 - 2 * m)), near);
    return sat16(((long long)far + (long long)near + 16384) >> 15, clips);
}
// Step 3.  codec 0 linear, 1 mu-law, 2 A-law: D[E(v)] of the "G.711 payloads" section.
__host__ __device__ inline int codec_of(int codec, int v) {
    if (codec == 1) return gtk::g711_decode(0, gtk::g711_encode(0, v));
    if (codec == 2) return gtk::g711_decode(1, gtk::g711_encode(1, v));
    return v;
}
// Step 4 for the four outputs i = 4t .. 4t + 3.  a[m] = pack2(w[2n], w[2n + 1]) at n = t - 16 + m and
// b[m] = pack2(w[2n - 1], w[2n]) at n = t - 15 + m, m = 0 .. 32: output 4t meets the even taps over `a`, 4t + 2 over `b`, and
// the odd taps serve 4t + 1 over `b` and 4t + 3 over `a` one pair on.  Zero-stuffed samples are never multiplied.  clip[q] is 1
// where output q was clipped.
__host__ __device__ inline void interpolate4(const uint32_t* a, const uint32_t* b, int* z, int* clip) {
    int e0 = 0, e2 = 0, o1 = 0, o3 = 0;
#pragma unroll
    for (int m = 0; m < 33; ++m) {
        const uint32_t te = pack2(tap(128 - 4 * m), tap(126 - 4 * m));
        e0 = dot2(a[m], te, e0);
        e2 = dot2(b[m], te, e2);
    }
#pragma unroll
    for (int m = 0; m < 32; ++m) {
        const uint32_t to = pack2(tap(127 - 4 * m), tap(125 - 4 * m));
        o1 = dot2(b[m], to, o1);
        o3 = dot2(a[m + 1], to, o3);
    }
    clip[0] = clip[1] = clip[2] = clip[3] = 0;
    z[0] = sat16(((long long)e0 + 8192) >> 14, clip + 0);
    z[1] = sat16(((long long)o1 + 8192) >> 14, clip + 1);
    z[2] = sat16(((long long)e2 + 8192) >> 14, clip + 2);
    z[3] = sat16(((long long)o3 + 8192) >> 14, clip + 3);
}
// Step 5: exact, |z| <= 2^15.
__host__ __device__ inline float out_of(int z) { return (float)z * 3.0517578125e-05f; }

// A plan entry as the channel uses it: anything outside -1 .. 2 is a wide-band row.
__host__ __device__ inline int codec_in_range(int c) { return c < -1 || c > 2 ? -1 : c; }

// Row b of a phone plan: Philox block k = 3 of the batch plan's counter and key.
__host__ __device__ inline PItem phone_item(float p_phone, int codec_mask, long item0, uint64_t seed, uint64_t step, int b) {
    uint32_t t[4];
    const uint32_t c0 = (uint32_t)((uint64_t)item0 + (uint64_t)b);
    gtb::philox4x32_10(c0, (uint32_t)step, (uint32_t)(step >> 32), 3u, (uint32_t)seed, (uint32_t)(seed >> 32), t);
    PItem it = {-1, 0};
    if (gtb::unit24(t[0]) < p_phone) {
        const int n = (codec_mask & 1) + ((codec_mask >> 1) & 1) + ((codec_mask >> 2) & 1);
        int k = (int)gtb::mulhi32(t[1], (uint32_t)n);   // the k-th set bit from the low end
        for (int c = 0; c < 3; ++c)
            if ((codec_mask >> c) & 1) {
                if (k == 0) { it.codec = c; break; }
                --k;
            }
    }
    return it;
}

// ---- the chunk geometry -----------------------------------------------------------------------------------------------------
// A workgroup writes CHUNK consecutive outputs of one row.  Their QUADS fours of outputs read the w pairs n = c0 / 4 - 16 ..
// c0 / 4 + QUADS + 16 (the `b` pairs are cut from those), VPAIRS pairs: three passes of the workgroup exactly.  Those pairs read
// the p pairs 2n - 32 .. 2n + 33, PPAIRS in all, from sample c0 - 128 on.
constexpr int THREADS = 256;
constexpr int VPAIRS = 3 * THREADS;
constexpr int QUADS = VPAIRS - 33;
constexpr int CHUNK = 4 * QUADS;                       // 2940
constexpr int PPAIRS = 2 * (VPAIRS - 1) + 66;          // 1600
static_assert(CHUNK % 4 == 0, "a chunk starts on a 16-byte boundary of its row");

struct PhoneArgs {
    const float* src[2] = {nullptr, nullptr};          // noisy, clean (clean may be null, then dst[1] is null too)
    float* dst[2] = {nullptr, nullptr};
    long src_stride[2] = {0, 0}, dst_stride[2] = {0, 0};
    const PItem* plan = nullptr;
    int B = 0;
    long L = 0;
    int target = 0;                                    // 0 narrow, 1 wide
    PRecord* rec = nullptr;
    int chunks = 0;                                    // launch_phone sets it
    bool vec = false;                                  // every row of every buffer starts on 16 bytes
};

__host__ __device__ inline int chunks_of(long L) { return (int)((L + CHUNK - 1) / CHUNK); }

// Every launch_* returns 0 or a hipError_t.
int launch_phone_plan(float p_phone, int codec_mask, int B, long item0, const unsigned long long* d_seed_step, PItem* d_plan,
                      hipStream_t s);
int launch_phone(PhoneArgs a, hipStream_t s);

}  // namespace gtp
