// batch_host.cpp -- the "training batches from a resident corpus" and "active levels" sections of include/gtcrn_micro_hip.h: argument checks,
// launch sequencing and gtcrn_batch_plan_host, the plan's own function body (batch.h) run on the host.  The kernels are in
// batch.hip.  Compiled with -ffp-contract=off like them.
#include "../../include/gtcrn_micro_hip.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "batch.h"

extern "C" void gtcrn_set_error_(const char* msg);   // api.cpp: thread-local last error

static_assert(sizeof(gtcrn_batch_item) == 32 && sizeof(gtb::Item) == 32, "the plan item is 32 bytes");
static_assert(sizeof(gtcrn_batch_record) == 40 && sizeof(gtb::Record) == 40, "the mix record is 40 bytes");

namespace {

int bfail(int code, const std::string& m) {
    gtcrn_set_error_(m.c_str());
    return code;
}

constexpr long long kMaxGrid = 0x7fffffffLL;

// the checks both plan entry points share; fills `a`
int plan_args(const std::string& w, const long long* soff, int n_speech, const long long* noff, int n_noise, int B, long L,
              long item0, int granule, float snr_lo, float snr_hi, float lvl_lo, float lvl_hi, const int* clips,
              const void* seed_step, const void* plan, gtb::PlanArgs* a) {
    if (B <= 0 || L <= 0 || L > gtb::MAX_L) return bfail(GTCRN_ERR_ARG, w + ": B and L must be positive (L below 2^31)");
    if (!soff || !seed_step || !plan) return bfail(GTCRN_ERR_ARG, w + ": null pointer");
    if (n_speech <= 0) return bfail(GTCRN_ERR_ARG, w + ": the corpus is empty");
    if (noff && n_noise <= 0) return bfail(GTCRN_ERR_ARG, w + ": the noise corpus is empty");
    if (granule < 1) return bfail(GTCRN_ERR_ARG, w + ": granule must be at least 1");
    if (!(snr_hi >= snr_lo) || !(lvl_hi >= lvl_lo)) return bfail(GTCRN_ERR_ARG, w + ": a range has hi < lo");
    if (item0 < 0 || (long long)item0 + B > (1LL << 32)) return bfail(GTCRN_ERR_ARG, w + ": item0 .. item0 + B must lie in 0 .. 2^32");
    a->soff = soff; a->noff = noff; a->n_speech = n_speech; a->n_noise = noff ? n_noise : 0;
    a->B = B; a->L = L; a->item0 = item0; a->granule = granule;
    a->snr_lo = snr_lo; a->snr_hi = snr_hi; a->lvl_lo = lvl_lo; a->lvl_hi = lvl_hi;
    a->clips = clips;
    return 0;
}

int draw_args(const std::string& w, const short* pa, const short* pb, const long long* offa, int na, const long long* offb, int nb,
              const gtcrn_batch_item* plan, int B, long L, float* noisy, long noisy_stride, float* clean, long clean_stride,
              gtb::DrawArgs* d) {
    if (B <= 0 || L <= 0 || L > gtb::MAX_L) return bfail(GTCRN_ERR_ARG, w + ": B and L must be positive (L below 2^31)");
    if (!pa || !pb || !offa || !offb || !plan || !noisy || !clean) return bfail(GTCRN_ERR_ARG, w + ": null pointer");
    if (na <= 0 || nb <= 0) return bfail(GTCRN_ERR_ARG, w + ": a corpus is empty");
    if (noisy_stride < L || clean_stride < L) return bfail(GTCRN_ERR_ARG, w + ": a stride is shorter than its row");
    if ((reinterpret_cast<uintptr_t>(noisy) & 3) || (reinterpret_cast<uintptr_t>(clean) & 3) || (reinterpret_cast<uintptr_t>(plan) & 3))
        return bfail(GTCRN_ERR_ARG, w + ": misaligned pointer");
    d->a.pcm = pa; d->a.off = offa; d->a.n = na;
    d->b.pcm = pb; d->b.off = offb; d->b.n = nb;
    d->plan = reinterpret_cast<const gtb::Item*>(plan);
    d->B = B; d->L = L;
    d->noisy = noisy; d->clean = clean; d->noisy_stride = noisy_stride; d->clean_stride = clean_stride;
    return 0;
}

}  // namespace

int gtcrn_batch_plan(const long long* d_speech_offsets, int n_speech, const long long* d_noise_offsets, int n_noise, int B, long L,
                     long item0, int granule, float snr_lo, float snr_hi, float lvl_lo, float lvl_hi, const int* d_clips,
                     unsigned long long* d_seed_step, int advance, gtcrn_batch_item* d_plan, void* stream) {
    const std::string w("gtcrn_batch_plan");
    gtb::PlanArgs a;
    const int rc = plan_args(w, d_speech_offsets, n_speech, d_noise_offsets, n_noise, B, L, item0, granule, snr_lo, snr_hi, lvl_lo,
                             lvl_hi, d_clips, d_seed_step, d_plan, &a);
    if (rc != 0) return rc;
    if ((reinterpret_cast<uintptr_t>(d_seed_step) & 7) || (reinterpret_cast<uintptr_t>(d_plan) & 3))
        return bfail(GTCRN_ERR_ARG, w + ": misaligned pointer");
    const int e = gtb::launch_plan(a, d_seed_step, advance, reinterpret_cast<gtb::Item*>(d_plan), static_cast<hipStream_t>(stream));
    if (e != 0) return bfail(GTCRN_ERR_HIP, w + ": " + hipGetErrorString(static_cast<hipError_t>(e)));
    return 0;
}

int gtcrn_batch_plan_host(const long long* h_speech_offsets, int n_speech, const long long* h_noise_offsets, int n_noise, int B,
                          long L, long item0, int granule, float snr_lo, float snr_hi, float lvl_lo, float lvl_hi,
                          const int* h_clips, const unsigned long long* h_seed_step, gtcrn_batch_item* h_plan) {
    gtb::PlanArgs a;
    const int rc = plan_args("gtcrn_batch_plan_host", h_speech_offsets, n_speech, h_noise_offsets, n_noise, B, L, item0, granule,
                             snr_lo, snr_hi, lvl_lo, lvl_hi, h_clips, h_seed_step, h_plan, &a);
    if (rc != 0) return rc;
    gtb::Item* out = reinterpret_cast<gtb::Item*>(h_plan);
    for (int b = 0; b < B; ++b) out[b] = gtb::plan_item(a, h_seed_step[0], h_seed_step[1], b);
    return 0;
}

size_t gtcrn_batch_workspace_bytes(int B, long L) {
    if (B <= 0 || L <= 0 || L > gtb::MAX_L || (long long)B * gtb::chunks_of(L) > kMaxGrid) {
        bfail(GTCRN_ERR_ARG, "gtcrn_batch_workspace_bytes: B and L must be positive, L below 2^31, B * chunks below 2^31");
        return 0;
    }
    const size_t cells = (size_t)B * (size_t)gtb::chunks_of(L);
    return (cells * (3 * sizeof(long long) + sizeof(float)) + 15) & ~(size_t)15;
}

int gtcrn_batch_pairs(const short* d_noisy_pcm, const short* d_clean_pcm, const long long* d_offsets, int n,
                      const gtcrn_batch_item* d_plan, int B, long L, float* d_noisy, long noisy_stride, float* d_clean,
                      long clean_stride, void* stream) {
    const std::string w("gtcrn_batch_pairs");
    gtb::DrawArgs d;
    const int rc = draw_args(w, d_noisy_pcm, d_clean_pcm, d_offsets, n, d_offsets, n, d_plan, B, L, d_noisy, noisy_stride, d_clean,
                             clean_stride, &d);
    if (rc != 0) return rc;
    if ((long long)B * ((L + gtb::TILE - 1) / gtb::TILE) > kMaxGrid) return bfail(GTCRN_ERR_ARG, w + ": B * L is too large for one launch");
    const int e = gtb::launch_pairs(d, static_cast<hipStream_t>(stream));
    if (e != 0) return bfail(GTCRN_ERR_HIP, w + ": " + hipGetErrorString(static_cast<hipError_t>(e)));
    return 0;
}

namespace {

// what every mix entry point checks after draw_args: the records, the workspace, the target corpus if one is given, `passes`
int mix_buffers(const std::string& w, const void* d_records, const void* d_workspace, const short* d_target_pcm, bool target_needed,
                int passes) {
    if (!d_records || !d_workspace || (target_needed && !d_target_pcm)) return bfail(GTCRN_ERR_ARG, w + ": null pointer");
    if (d_target_pcm && (reinterpret_cast<uintptr_t>(d_target_pcm) & 1)) return bfail(GTCRN_ERR_ARG, w + ": misaligned pointer");
    if ((reinterpret_cast<uintptr_t>(d_records) & 7) || (reinterpret_cast<uintptr_t>(d_workspace) & 15))
        return bfail(GTCRN_ERR_ARG, w + ": the records must be 8-byte, the workspace 16-byte aligned");
    if (passes < 1 || passes > 7) return bfail(GTCRN_ERR_ARG, w + ": `passes` is a sum of 1 (sums), 2 (peak) and 4 (write); 7 is a draw");
    return 0;
}

// gtcrn_batch_mix (d_target_pcm null) and gtcrn_batch_mix_target: one set of checks, two launch sequences
int mix_call(const std::string& w, const short* d_speech_pcm, const long long* d_speech_offsets, int n_speech,
             const short* d_noise_pcm, const long long* d_noise_offsets, int n_noise, const short* d_target_pcm, bool with_target,
             const gtcrn_batch_item* d_plan, int B, long L, float* d_noisy, long noisy_stride, float* d_clean, long clean_stride,
             gtcrn_batch_record* d_records, void* d_workspace, int passes, void* stream) {
    gtb::DrawArgs d;
    const int rc = draw_args(w, d_speech_pcm, d_noise_pcm, d_speech_offsets, n_speech, d_noise_offsets, n_noise, d_plan, B, L, d_noisy,
                             noisy_stride, d_clean, clean_stride, &d);
    if (rc != 0) return rc;
    const int rb = mix_buffers(w, d_records, d_workspace, d_target_pcm, with_target, passes);
    if (rb != 0) return rb;
    const long long cells = (long long)B * gtb::chunks_of(L);
    if (cells > kMaxGrid) return bfail(GTCRN_ERR_ARG, w + ": B * L is too large for one launch");
    d.rec = reinterpret_cast<gtb::Record*>(d_records);
    d.sums = static_cast<long long*>(d_workspace);
    d.peaks = reinterpret_cast<float*>(d.sums + 3 * cells);
    const int e = with_target ? gtb::launch_mix_target(d, d_target_pcm, passes, static_cast<hipStream_t>(stream))
                              : gtb::launch_mix(d, passes, static_cast<hipStream_t>(stream));
    if (e != 0) return bfail(GTCRN_ERR_HIP, w + ": " + hipGetErrorString(static_cast<hipError_t>(e)));
    return 0;
}

}  // namespace

int gtcrn_batch_mix(const short* d_speech_pcm, const long long* d_speech_offsets, int n_speech, const short* d_noise_pcm,
                    const long long* d_noise_offsets, int n_noise, const gtcrn_batch_item* d_plan, int B, long L, float* d_noisy,
                    long noisy_stride, float* d_clean, long clean_stride, gtcrn_batch_record* d_records, void* d_workspace,
                    int passes, void* stream) {
    return mix_call("gtcrn_batch_mix", d_speech_pcm, d_speech_offsets, n_speech, d_noise_pcm, d_noise_offsets, n_noise, nullptr, false,
                    d_plan, B, L, d_noisy, noisy_stride, d_clean, clean_stride, d_records, d_workspace, passes, stream);
}

int gtcrn_batch_mix_target(const short* d_speech_pcm, const long long* d_speech_offsets, int n_speech, const short* d_noise_pcm,
                           const long long* d_noise_offsets, int n_noise, const short* d_target_pcm, const gtcrn_batch_item* d_plan,
                           int B, long L, float* d_noisy, long noisy_stride, float* d_clean, long clean_stride,
                           gtcrn_batch_record* d_records, void* d_workspace, int passes, void* stream) {
    return mix_call("gtcrn_batch_mix_target", d_speech_pcm, d_speech_offsets, n_speech, d_noise_pcm, d_noise_offsets, n_noise,
                    d_target_pcm, true, d_plan, B, L, d_noisy, noisy_stride, d_clean, clean_stride, d_records, d_workspace, passes,
                    stream);
}

// ---- active levels ------------------------------------------------------------------------------------------------------------

static_assert(sizeof(gtcrn_batch_active_record) == 64 && sizeof(gtb::ActiveRecord) == 64, "the active record is 64 bytes");

namespace {

bool window_ok(int window) { return window >= gtb::MIN_WINDOW && window <= gtb::MAX_WINDOW && window % gtb::GROUP == 0; }

}  // namespace

size_t gtcrn_batch_active_workspace_bytes(int B, long L, int window) {
    if (B <= 0 || L <= 0 || L > gtb::MAX_L || !window_ok(window) || (long long)B * gtb::active_chunks_of(L, window) > kMaxGrid) {
        bfail(GTCRN_ERR_ARG, "gtcrn_batch_active_workspace_bytes: B and L must be positive, L below 2^31, window a multiple of 8 in "
                             "8 .. 2^20, B * chunks below 2^31");
        return 0;
    }
    const size_t cells = (size_t)B * (size_t)gtb::active_chunks_of(L, window);
    return (cells * (gtb::ACTIVE_PARTS * sizeof(long long) + sizeof(float)) + 15) & ~(size_t)15;
}

int gtcrn_batch_mix_active(const short* d_speech_pcm, const long long* d_speech_offsets, int n_speech, const short* d_noise_pcm,
                           const long long* d_noise_offsets, int n_noise, const short* d_target_pcm, const gtcrn_batch_item* d_plan,
                           int B, long L, float* d_noisy, long noisy_stride, float* d_clean, long clean_stride, int window,
                           long long threshold, gtcrn_batch_active_record* d_records, void* d_workspace, int passes, void* stream) {
    const std::string w("gtcrn_batch_mix_active");
    gtb::DrawArgs d;
    const int rc = draw_args(w, d_speech_pcm, d_noise_pcm, d_speech_offsets, n_speech, d_noise_offsets, n_noise, d_plan, B, L, d_noisy,
                             noisy_stride, d_clean, clean_stride, &d);
    if (rc != 0) return rc;
    const int rb = mix_buffers(w, d_records, d_workspace, d_target_pcm, false, passes);
    if (rb != 0) return rb;
    if (!window_ok(window)) return bfail(GTCRN_ERR_ARG, w + ": `window` is a multiple of 8 samples in 8 .. 2^20");
    if (threshold < 0 || threshold > gtb::MAX_THRESHOLD) return bfail(GTCRN_ERR_ARG, w + ": `threshold` lies in 0 .. 2^30");
    const long long cells = (long long)B * gtb::active_chunks_of(L, window);
    if (cells > kMaxGrid) return bfail(GTCRN_ERR_ARG, w + ": B * L is too large for one launch");
    d.sums = static_cast<long long*>(d_workspace);
    d.peaks = reinterpret_cast<float*>(d.sums + gtb::ACTIVE_PARTS * cells);
    const int e = gtb::launch_mix_active(d, d_target_pcm, reinterpret_cast<gtb::ActiveRecord*>(d_records), window, threshold, passes,
                                         static_cast<hipStream_t>(stream));
    if (e != 0) return bfail(GTCRN_ERR_HIP, w + ": " + hipGetErrorString(static_cast<hipError_t>(e)));
    return 0;
}
