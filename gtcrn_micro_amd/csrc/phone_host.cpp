// phone_host.cpp -- the "telephone-channel rows: exact 8 kHz band + G.711" section of include/gtcrn_micro_hip.h: the table's
// design, argument checks, launch sequencing, and the host twins gtcrn_batch_phone_plan_host and gtcrn_batch_phone_host, which
// run phone.h's own functions -- the ones phone.hip compiles for the device -- row by row on host pointers.  Compiled with
// -ffp-contract=off like batch_host.cpp.
#include "../../include/gtcrn_micro_hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "phone.h"

extern "C" void gtcrn_set_error_(const char* msg);   // api.cpp: thread-local last error

static_assert(sizeof(gtcrn_phone_item) == 8 && sizeof(gtp::PItem) == 8, "the phone plan item is 8 bytes");
static_assert(sizeof(gtcrn_phone_record) == 16 && sizeof(gtp::PRecord) == 16, "the phone record is 16 bytes");
static_assert(GTCRN_PHONE_TAPS == gtp::NTAPS, "the header states the table's length");

namespace {

int pfail(int code, const std::string& m) {
    gtcrn_set_error_(m.c_str());
    return code;
}

constexpr long long kMaxGrid = 0x7fffffffLL;

double bessel_i0(double x) {        // sum over k of ((x / 2)^k / k!)^2, as the resampler's design has it
    const double y = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= y / ((double)k * (double)k);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}

// The 16 kHz -> 8 kHz design of "sample-rate conversion" (q = 2, half = 64, sum(h) = 1) in double, then rint(32768 h[n]).
// No 32768 h[n] lies within 0.003 of a rounding tie, so this and any other double design agree on every entry.
void design_taps(int* t) {
    const int half = gtp::HALF, n = gtp::NTAPS;
    const double kPi = 3.14159265358979323846, beta = 8.95926, fc = 0.9375 * 0.5 / 2.0, i0b = bessel_i0(beta);
    double h[gtp::NTAPS], sum = 0.0;
    for (int i = 0; i < n; ++i) {
        const int k = i - half;
        const double y = kPi * 2.0 * fc * k, r = (double)k / (double)half;
        h[i] = (k == 0 ? 1.0 : std::sin(y) / y) * (bessel_i0(beta * std::sqrt(1.0 - r * r)) / i0b);
        sum += h[i];
    }
    for (int i = 0; i < n; ++i) t[i] = (int)std::rint(32768.0 * (h[i] / sum));
}

int plan_args(const std::string& w, float p, int mask, int B, long item0, const void* seed_step, const void* plan) {
    if (B <= 0) return pfail(GTCRN_ERR_ARG, w + ": B must be positive");
    if (!(p >= 0.0f && p <= 1.0f)) return pfail(GTCRN_ERR_ARG, w + ": p_phone must lie in 0 .. 1");
    if (mask < 1 || mask > 7) return pfail(GTCRN_ERR_ARG, w + ": codec_mask must lie in 1 .. 7 (bit 0 linear, 1 mu-law, 2 A-law)");
    if (!seed_step || !plan) return pfail(GTCRN_ERR_ARG, w + ": null pointer");
    if (item0 < 0 || (long long)item0 + B > (1LL << 32)) return pfail(GTCRN_ERR_ARG, w + ": item0 .. item0 + B must lie in 0 .. 2^32");
    if ((reinterpret_cast<uintptr_t>(seed_step) & 7) || (reinterpret_cast<uintptr_t>(plan) & 3))
        return pfail(GTCRN_ERR_ARG, w + ": misaligned pointer");
    return 0;
}

// [first byte, one past the last byte) of B rows of L floats at a stride
struct Range { uintptr_t lo, hi; };
Range range_of(const void* p, long stride, int B, long L) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    return {lo, lo + ((uintptr_t)(B - 1) * (uintptr_t)stride + (uintptr_t)L) * sizeof(float)};
}
bool overlap(Range a, Range b) { return a.lo < b.hi && b.lo < a.hi; }

// the checks gtcrn_batch_phone and gtcrn_batch_phone_host share; fills `a`
int phone_args(const std::string& w, const float* src_noisy, long src_noisy_stride, const float* src_clean, long src_clean_stride,
               const gtcrn_phone_item* plan, int B, long L, float* noisy, long noisy_stride, float* clean, long clean_stride,
               int target, gtcrn_phone_record* records, gtp::PhoneArgs* a) {
    if (B <= 0 || L <= 0 || L > gtb::MAX_L) return pfail(GTCRN_ERR_ARG, w + ": B and L must be positive (L below 2^31)");
    if (!src_noisy || !noisy || !plan || !records) return pfail(GTCRN_ERR_ARG, w + ": null pointer");
    if ((src_clean == nullptr) != (clean == nullptr))
        return pfail(GTCRN_ERR_ARG, w + ": the clean source and the clean output are both given or both NULL");
    if (target != 0 && target != 1) return pfail(GTCRN_ERR_ARG, w + ": target is 0 (narrow) or 1 (wide)");
    if (src_noisy_stride < L || noisy_stride < L || (clean && (src_clean_stride < L || clean_stride < L)))
        return pfail(GTCRN_ERR_ARG, w + ": a stride is shorter than its row");
    if ((reinterpret_cast<uintptr_t>(src_noisy) | reinterpret_cast<uintptr_t>(noisy) | reinterpret_cast<uintptr_t>(src_clean) |
         reinterpret_cast<uintptr_t>(clean) | reinterpret_cast<uintptr_t>(plan) | reinterpret_cast<uintptr_t>(records)) & 3)
        return pfail(GTCRN_ERR_ARG, w + ": misaligned pointer");
    if ((long long)B * gtp::chunks_of(L) > kMaxGrid) return pfail(GTCRN_ERR_ARG, w + ": B * L is too large for one launch");
    const Range s0 = range_of(src_noisy, src_noisy_stride, B, L), d0 = range_of(noisy, noisy_stride, B, L);
    bool bad = overlap(s0, d0);
    if (clean) {
        const Range s1 = range_of(src_clean, src_clean_stride, B, L), d1 = range_of(clean, clean_stride, B, L);
        bad = bad || overlap(s0, d1) || overlap(s1, d0) || overlap(s1, d1) || overlap(d0, d1);
    }
    if (bad) return pfail(GTCRN_ERR_ARG, w + ": a source range overlaps a destination range (the halo reads make in-place use a race)");
    a->src[0] = src_noisy; a->src[1] = src_clean;
    a->dst[0] = noisy; a->dst[1] = clean;
    a->src_stride[0] = src_noisy_stride; a->src_stride[1] = src_clean_stride;
    a->dst_stride[0] = noisy_stride; a->dst_stride[1] = clean_stride;
    a->plan = reinterpret_cast<const gtp::PItem*>(plan);
    a->B = B; a->L = L; a->target = target;
    a->rec = reinterpret_cast<gtp::PRecord*>(records);
    a->chunks = gtp::chunks_of(L);
    uintptr_t bits = reinterpret_cast<uintptr_t>(src_noisy) | reinterpret_cast<uintptr_t>(noisy) | ((uintptr_t)src_noisy_stride * 4) |
                     ((uintptr_t)noisy_stride * 4);
    if (clean)
        bits |= reinterpret_cast<uintptr_t>(src_clean) | reinterpret_cast<uintptr_t>(clean) | ((uintptr_t)src_clean_stride * 4) |
                ((uintptr_t)clean_stride * 4);
    a->vec = (bits & 15) == 0;
    return 0;
}

// One row through steps 1 - 5 on the host: the whole row as one chunk.  clips (may be null): {step 2, step 4}.
void channel_row(const float* src, float* dst, long L, int codec, int* clips) {
    const long J = (L + 1) / 2, NP = (J + 1) / 2, Q = (L + 3) / 4;     // v values, their pairs, fours of outputs
    // p pairs from sample -64 on: v[j] reads the pairs j .. j + 64
    std::vector<uint32_t> p((size_t)J + 66, 0u);
    for (long d = 0; d < (L + 1) / 2; ++d) {
        const long i = 2 * d;
        p[(size_t)d + 32] = gtp::pack2(gtp::pcm_of(src[i]), i + 1 < L ? gtp::pcm_of(src[i + 1]) : 0);
    }
    // w pairs a[n + 16] = (w[2n], w[2n + 1]) and b[n + 16] = (w[2n - 1], w[2n]), n = -16 .. Q + 17, zero outside the row
    std::vector<uint32_t> a((size_t)Q + 34, 0u), b((size_t)Q + 34, 0u);
    int down = 0, up = 0;
    for (long n = 0; n < NP; ++n) {
        int w[2] = {0, 0};
        for (int e = 0; e < 2; ++e) {
            const long j = 2 * n + e;
            if (j < J) w[e] = gtp::codec_of(codec, gtp::decimate_at(p.data() + j, &down));
        }
        a[(size_t)n + 16] = gtp::pack2(w[0], w[1]);
    }
    for (size_t k = 1; k < a.size(); ++k) b[k] = (a[k - 1] >> 16) | (a[k] << 16);
    for (long t = 0; t < Q; ++t) {
        int z[4], clip[4];
        gtp::interpolate4(a.data() + t, b.data() + t + 1, z, clip);
        for (int q = 0; q < 4; ++q)
            if (4 * t + q < L) {
                dst[4 * t + q] = gtp::out_of(z[q]);
                up += clip[q];
            }
    }
    if (clips) { clips[0] = down; clips[1] = up; }
}

}  // namespace

int gtcrn_batch_phone_taps(int* h_taps) {
    if (!h_taps) return pfail(GTCRN_ERR_ARG, "gtcrn_batch_phone_taps: null pointer");
    int t[gtp::NTAPS];
    design_taps(t);
    for (int k = 0; k < gtp::NTAPS; ++k) {
        if (t[k] != gtp::tap(k))
            return pfail(GTCRN_ERR_STATE, "gtcrn_batch_phone_taps: the designed table differs from the compiled one at entry " +
                                              std::to_string(k));
        h_taps[k] = gtp::tap(k);
    }
    return gtp::NTAPS;
}

int gtcrn_batch_phone_chunk(void) { return gtp::CHUNK; }

int gtcrn_batch_phone_plan(float p_phone, int codec_mask, int B, long item0, const unsigned long long* d_seed_step,
                           gtcrn_phone_item* d_plan, void* stream) {
    const std::string w("gtcrn_batch_phone_plan");
    const int rc = plan_args(w, p_phone, codec_mask, B, item0, d_seed_step, d_plan);
    if (rc != 0) return rc;
    const int e = gtp::launch_phone_plan(p_phone, codec_mask, B, item0, d_seed_step, reinterpret_cast<gtp::PItem*>(d_plan),
                                         static_cast<hipStream_t>(stream));
    if (e != 0) return pfail(GTCRN_ERR_HIP, w + ": " + hipGetErrorString(static_cast<hipError_t>(e)));
    return 0;
}

int gtcrn_batch_phone_plan_host(float p_phone, int codec_mask, int B, long item0, const unsigned long long* h_seed_step,
                                gtcrn_phone_item* h_plan) {
    const int rc = plan_args("gtcrn_batch_phone_plan_host", p_phone, codec_mask, B, item0, h_seed_step, h_plan);
    if (rc != 0) return rc;
    gtp::PItem* out = reinterpret_cast<gtp::PItem*>(h_plan);
    for (int b = 0; b < B; ++b) out[b] = gtp::phone_item(p_phone, codec_mask, item0, h_seed_step[0], h_seed_step[1], b);
    return 0;
}

int gtcrn_batch_phone(const float* d_src_noisy, long src_noisy_stride, const float* d_src_clean, long src_clean_stride,
                      const gtcrn_phone_item* d_plan, int B, long L, float* d_noisy, long noisy_stride, float* d_clean,
                      long clean_stride, int target, gtcrn_phone_record* d_records, void* stream) {
    const std::string w("gtcrn_batch_phone");
    gtp::PhoneArgs a;
    const int rc = phone_args(w, d_src_noisy, src_noisy_stride, d_src_clean, src_clean_stride, d_plan, B, L, d_noisy, noisy_stride,
                              d_clean, clean_stride, target, d_records, &a);
    if (rc != 0) return rc;
    const int e = gtp::launch_phone(a, static_cast<hipStream_t>(stream));
    if (e != 0) return pfail(GTCRN_ERR_HIP, w + ": " + hipGetErrorString(static_cast<hipError_t>(e)));
    return 0;
}

int gtcrn_batch_phone_host(const float* h_src_noisy, long src_noisy_stride, const float* h_src_clean, long src_clean_stride,
                           const gtcrn_phone_item* h_plan, int B, long L, float* h_noisy, long noisy_stride, float* h_clean,
                           long clean_stride, int target, gtcrn_phone_record* h_records) {
    gtp::PhoneArgs a;
    const int rc = phone_args("gtcrn_batch_phone_host", h_src_noisy, src_noisy_stride, h_src_clean, src_clean_stride, h_plan, B, L,
                              h_noisy, noisy_stride, h_clean, clean_stride, target, h_records, &a);
    if (rc != 0) return rc;
    for (int b = 0; b < B; ++b) {
        const int codec = gtp::codec_in_range(a.plan[b].codec);
        gtp::PRecord rec = {codec, 0, 0, 0};
        for (int side = 0; side < (a.src[1] ? 2 : 1); ++side) {
            const float* src = a.src[side] + (long long)b * a.src_stride[side];
            float* dst = a.dst[side] + (long long)b * a.dst_stride[side];
            if (codec < 0 || (side == 1 && target == 1)) {
                std::memcpy(dst, src, (size_t)L * sizeof(float));
            } else {
                int clips[2];
                channel_row(src, dst, L, side == 1 ? 0 : codec, clips);
                if (side == 0) { rec.saturated_down = clips[0]; rec.saturated_up = clips[1]; }
            }
        }
        a.rec[b] = rec;
    }
    return 0;
}
