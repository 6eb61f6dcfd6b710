// reverb_host.cpp -- the "reverberant speech: exact RIR convolution" section of include/gtcrn_micro_hip.h: argument checks,
// launch sequencing, gtcrn_batch_reverb_plan_host (the reverb plan's own function body, reverb.h, run on the host) and the
// host side of gtcrn_selftest_mfma_i8; behind them the "dereverberation targets: early or direct clean" section (the split
// convolution).  The kernels are in reverb.hip.  Compiled with -ffp-contract=off like batch_host.cpp.
#include "../../include/gtcrn_micro_hip.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "reverb.h"

extern "C" void gtcrn_set_error_(const char* msg);   // api.cpp: thread-local last error

static_assert(sizeof(gtcrn_reverb_item) == 8 && sizeof(gtr::RItem) == 8, "the reverb plan item is 8 bytes");
static_assert(sizeof(gtcrn_reverb_record) == 16 && sizeof(gtr::RRecord) == 16, "the reverb record is 16 bytes");
static_assert(sizeof(gtcrn_reverb_split_record) == 32 && sizeof(gtr::SRecord) == 32, "the split record is 32 bytes");
static_assert(GTCRN_REVERB_MAX_TAPS == gtr::MAX_TAPS && GTCRN_REVERB_TAP_MAX == gtr::TAP_MAX, "the header states the bank's bounds");

namespace {

int rfail(int code, const std::string& m) {
    gtcrn_set_error_(m.c_str());
    return code;
}

constexpr long long kMaxGrid = 0x7fffffffLL;

long long blocks_of(long L) { return ((long long)L + gtr::BLOCK - 1) / gtr::BLOCK; }

int rplan_args(const std::string& w, int n_rir, float p, int B, long item0, const void* seed_step, const void* rplan) {
    if (B <= 0) return rfail(GTCRN_ERR_ARG, w + ": B must be positive");
    if (n_rir <= 0) return rfail(GTCRN_ERR_ARG, w + ": the bank is empty");
    if (!(p >= 0.0f && p <= 1.0f)) return rfail(GTCRN_ERR_ARG, w + ": p_reverb must lie in 0 .. 1");
    if (!seed_step || !rplan) return rfail(GTCRN_ERR_ARG, w + ": null pointer");
    if (item0 < 0 || (long long)item0 + B > (1LL << 32)) return rfail(GTCRN_ERR_ARG, w + ": item0 .. item0 + B must lie in 0 .. 2^32");
    if ((reinterpret_cast<uintptr_t>(seed_step) & 7) || (reinterpret_cast<uintptr_t>(rplan) & 3))
        return rfail(GTCRN_ERR_ARG, w + ": misaligned pointer");
    return 0;
}

struct DevMem {
    void* p = nullptr;
    ~DevMem() { if (p) (void)hipFree(p); }
};
struct DeviceScope {
    int prev = -1;
    DeviceScope() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

}  // namespace

int gtcrn_batch_reverb_plan(int n_rir, float p_reverb, int B, long item0, const unsigned long long* d_seed_step,
                            gtcrn_reverb_item* d_rplan, void* stream) {
    const std::string w("gtcrn_batch_reverb_plan");
    const int rc = rplan_args(w, n_rir, p_reverb, B, item0, d_seed_step, d_rplan);
    if (rc != 0) return rc;
    const int e = gtr::launch_reverb_plan(n_rir, p_reverb, B, item0, d_seed_step, reinterpret_cast<gtr::RItem*>(d_rplan),
                                          static_cast<hipStream_t>(stream));
    if (e != 0) return rfail(GTCRN_ERR_HIP, w + ": " + hipGetErrorString(static_cast<hipError_t>(e)));
    return 0;
}

int gtcrn_batch_reverb_plan_host(int n_rir, float p_reverb, int B, long item0, const unsigned long long* h_seed_step,
                                 gtcrn_reverb_item* h_rplan) {
    const int rc = rplan_args("gtcrn_batch_reverb_plan_host", n_rir, p_reverb, B, item0, h_seed_step, h_rplan);
    if (rc != 0) return rc;
    gtr::RItem* out = reinterpret_cast<gtr::RItem*>(h_rplan);
    for (int b = 0; b < B; ++b) out[b] = gtr::reverb_item(n_rir, p_reverb, item0, h_seed_step[0], h_seed_step[1], b);
    return 0;
}

size_t gtcrn_batch_reverb_table_bytes(const long long* h_rir_offsets, int n_rir) {
    if (!h_rir_offsets || n_rir <= 0) {
        rfail(GTCRN_ERR_ARG, "gtcrn_batch_reverb_table_bytes: a host offsets table of a bank that is not empty");
        return 0;
    }
    long long bytes = gtr::header_bytes(n_rir);
    for (int r = 0; r < n_rir; ++r) {
        const long long len = h_rir_offsets[r + 1] - h_rir_offsets[r];
        if (len < 1 || len > gtr::MAX_TAPS) {
            rfail(GTCRN_ERR_ARG, "gtcrn_batch_reverb_table_bytes: response " + std::to_string(r) + " has " + std::to_string(len) +
                                     " taps; 1 .. 16384 are allowed");
            return 0;
        }
        bytes += (long long)gtr::groups_of((int)len) * gtr::GROUP_BYTES;
    }
    return (size_t)bytes;
}

int gtcrn_batch_reverb_prepare(const short* d_taps, const long long* d_rir_offsets, int n_rir, void* d_table, size_t table_bytes,
                               void* stream) {
    const std::string w("gtcrn_batch_reverb_prepare");
    if (!d_taps || !d_rir_offsets || !d_table) return rfail(GTCRN_ERR_ARG, w + ": null pointer");
    if (n_rir <= 0) return rfail(GTCRN_ERR_ARG, w + ": the bank is empty");
    if (reinterpret_cast<uintptr_t>(d_table) & 15) return rfail(GTCRN_ERR_ARG, w + ": the table must be 16-byte aligned");
    const long long least = gtr::header_bytes(n_rir) + (long long)n_rir * gtr::groups_of(1) * gtr::GROUP_BYTES;
    const long long groups = ((long long)table_bytes - gtr::header_bytes(n_rir)) / gtr::GROUP_BYTES;
    if ((long long)table_bytes < least || groups > kMaxGrid)
        return rfail(GTCRN_ERR_ARG, w + ": table_bytes is not gtcrn_batch_reverb_table_bytes of a bank of this size");
    const int e = gtr::launch_reverb_prepare(d_taps, d_rir_offsets, n_rir, static_cast<unsigned char*>(d_table), (long long)table_bytes,
                                             static_cast<hipStream_t>(stream));
    if (e != 0) return rfail(GTCRN_ERR_HIP, w + ": " + hipGetErrorString(static_cast<hipError_t>(e)));
    return 0;
}

size_t gtcrn_batch_reverb_workspace_bytes(int B, long L) {
    if (B <= 0 || L <= 0 || L > gtb::MAX_L || (long long)B * blocks_of(L) > kMaxGrid) {
        rfail(GTCRN_ERR_ARG, "gtcrn_batch_reverb_workspace_bytes: B and L must be positive, L below 2^31, B * blocks below 2^31");
        return 0;
    }
    return ((size_t)B * (size_t)blocks_of(L) * sizeof(int) + 15) & ~(size_t)15;
}

namespace {

// the checks gtcrn_batch_reverb and gtcrn_batch_reverb_split share; fills `a` (but a.rec) and resolves form 0
int reverb_args(const std::string& w, const short* d_speech_pcm, const long long* d_speech_offsets, int n_speech, const short* d_taps,
                const long long* d_rir_offsets, int n_rir, const void* d_table, size_t table_bytes, long long header,
                const gtcrn_batch_item* d_plan, const gtcrn_reverb_item* d_rplan, int B, long L, short* d_staged, long staged_stride,
                long long* d_staged_offsets, gtcrn_batch_item* d_staged_plan, const void* d_records, void* d_workspace, int* form,
                gtr::ReverbArgs* a) {
    if (B <= 0 || L <= 0 || L > gtb::MAX_L) return rfail(GTCRN_ERR_ARG, w + ": B and L must be positive (L below 2^31)");
    if (!d_speech_pcm || !d_speech_offsets || !d_taps || !d_rir_offsets || !d_plan || !d_rplan || !d_staged || !d_staged_offsets ||
        !d_staged_plan || !d_records || !d_workspace)
        return rfail(GTCRN_ERR_ARG, w + ": null pointer");
    if (n_speech <= 0 || n_rir <= 0) return rfail(GTCRN_ERR_ARG, w + ": the corpus or the bank is empty");
    if (staged_stride < L) return rfail(GTCRN_ERR_ARG, w + ": the staged stride is shorter than its row");
    if (*form < 0 || *form > 4)
        return rfail(GTCRN_ERR_ARG, w + ": form is 0 (the library chooses), 1 (plain), 2 (matrix) or 3 / 4 (matrix, block pinned)");
    if (*form == 0) *form = 2;                        // the matrix form is the faster wherever both were measured
    if (*form >= 2) {
        if (!d_table) return rfail(GTCRN_ERR_ARG, w + ": the matrix form needs its table");
        if ((reinterpret_cast<uintptr_t>(d_table) & 15) || (long long)table_bytes < header)
            return rfail(GTCRN_ERR_ARG, w + ": the table must be 16-byte aligned and hold its header");
    }
    if ((reinterpret_cast<uintptr_t>(d_plan) & 3) || (reinterpret_cast<uintptr_t>(d_rplan) & 3) ||
        (reinterpret_cast<uintptr_t>(d_staged_plan) & 3) || (reinterpret_cast<uintptr_t>(d_records) & 3) ||
        (reinterpret_cast<uintptr_t>(d_workspace) & 3) || (reinterpret_cast<uintptr_t>(d_staged_offsets) & 7) ||
        (reinterpret_cast<uintptr_t>(d_staged) & 1))
        return rfail(GTCRN_ERR_ARG, w + ": misaligned pointer");
    if ((long long)B * blocks_of(L) > kMaxGrid) return rfail(GTCRN_ERR_ARG, w + ": B * L is too large for one launch");
    a->speech.pcm = d_speech_pcm; a->speech.off = d_speech_offsets; a->speech.n = n_speech;
    a->taps = d_taps; a->roff = d_rir_offsets; a->n_rir = n_rir;
    a->table = static_cast<const unsigned char*>(d_table); a->table_bytes = (long long)table_bytes;
    a->plan = reinterpret_cast<const gtb::Item*>(d_plan);
    a->rplan = reinterpret_cast<const gtr::RItem*>(d_rplan);
    a->B = B; a->L = L;
    a->staged = d_staged; a->stride = staged_stride; a->soffsets = d_staged_offsets;
    a->splan = reinterpret_cast<gtb::Item*>(d_staged_plan);
    a->partial = static_cast<int*>(d_workspace);
    a->blocks = 0;                                    // (launch_reverb / launch_split: the form's own block)
    return 0;
}

}  // namespace

int gtcrn_batch_reverb(const short* d_speech_pcm, const long long* d_speech_offsets, int n_speech, const short* d_taps,
                       const long long* d_rir_offsets, int n_rir, const void* d_table, size_t table_bytes,
                       const gtcrn_batch_item* d_plan, const gtcrn_reverb_item* d_rplan, int B, long L, short* d_staged,
                       long staged_stride, long long* d_staged_offsets, gtcrn_batch_item* d_staged_plan,
                       gtcrn_reverb_record* d_records, void* d_workspace, int form, void* stream) {
    const std::string w("gtcrn_batch_reverb");
    gtr::ReverbArgs a;
    const int rc = reverb_args(w, d_speech_pcm, d_speech_offsets, n_speech, d_taps, d_rir_offsets, n_rir, d_table, table_bytes,
                               gtr::header_bytes(n_rir), d_plan, d_rplan, B, L, d_staged, staged_stride, d_staged_offsets,
                               d_staged_plan, d_records, d_workspace, &form, &a);
    if (rc != 0) return rc;
    a.rec = reinterpret_cast<gtr::RRecord*>(d_records);
    const int e = gtr::launch_reverb(a, form, static_cast<hipStream_t>(stream));
    if (e != 0) return rfail(GTCRN_ERR_HIP, w + ": " + hipGetErrorString(static_cast<hipError_t>(e)));
    return 0;
}

// ---- dereverberation targets: the split convolution ---------------------------------------------------------------------------
size_t gtcrn_batch_reverb_split_table_bytes(const long long* h_rir_offsets, const int* h_split, int n_rir) {
    const std::string w("gtcrn_batch_reverb_split_table_bytes");
    if (!h_rir_offsets || !h_split || n_rir <= 0) {
        rfail(GTCRN_ERR_ARG, w + ": host offsets and splits of a bank that is not empty");
        return 0;
    }
    long long bytes = gtr::split_header_bytes(n_rir);
    for (int r = 0; r < n_rir; ++r) {
        const long long len = h_rir_offsets[r + 1] - h_rir_offsets[r];
        if (len < 1 || len > gtr::MAX_TAPS) {
            rfail(GTCRN_ERR_ARG, w + ": response " + std::to_string(r) + " has " + std::to_string(len) + " taps; 1 .. 16384 are allowed");
            return 0;
        }
        const int E = gtr::split_of(h_split[r], (int)len);
        bytes += (long long)(gtr::groups_of(E) + gtr::rest_groups(E, (int)len)) * gtr::GROUP_BYTES;
    }
    return (size_t)bytes;
}

int gtcrn_batch_reverb_split_prepare(const short* d_taps, const long long* d_rir_offsets, const int* d_split, int n_rir, void* d_table,
                                     size_t table_bytes, void* stream) {
    const std::string w("gtcrn_batch_reverb_split_prepare");
    if (!d_taps || !d_rir_offsets || !d_split || !d_table) return rfail(GTCRN_ERR_ARG, w + ": null pointer");
    if (n_rir <= 0) return rfail(GTCRN_ERR_ARG, w + ": the bank is empty");
    if (reinterpret_cast<uintptr_t>(d_table) & 15) return rfail(GTCRN_ERR_ARG, w + ": the table must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_split) & 3) return rfail(GTCRN_ERR_ARG, w + ": misaligned pointer");
    const long long least = gtr::split_header_bytes(n_rir) + (long long)n_rir * gtr::groups_of(1) * gtr::GROUP_BYTES;
    const long long groups = ((long long)table_bytes - gtr::split_header_bytes(n_rir)) / gtr::GROUP_BYTES;
    if ((long long)table_bytes < least || groups > kMaxGrid)
        return rfail(GTCRN_ERR_ARG, w + ": table_bytes is not gtcrn_batch_reverb_split_table_bytes of a bank of this size");
    const int e = gtr::launch_split_prepare(d_taps, d_rir_offsets, d_split, n_rir, static_cast<unsigned char*>(d_table),
                                            (long long)table_bytes, static_cast<hipStream_t>(stream));
    if (e != 0) return rfail(GTCRN_ERR_HIP, w + ": " + hipGetErrorString(static_cast<hipError_t>(e)));
    return 0;
}

size_t gtcrn_batch_reverb_split_workspace_bytes(int B, long L) {
    if (B <= 0 || L <= 0 || L > gtb::MAX_L || (long long)B * blocks_of(L) > kMaxGrid) {
        rfail(GTCRN_ERR_ARG, "gtcrn_batch_reverb_split_workspace_bytes: B and L must be positive, L below 2^31, B * blocks below 2^31");
        return 0;
    }
    return (2 * (size_t)B * (size_t)blocks_of(L) * sizeof(int) + 15) & ~(size_t)15;
}

int gtcrn_batch_reverb_split(const short* d_speech_pcm, const long long* d_speech_offsets, int n_speech, const short* d_taps,
                             const long long* d_rir_offsets, const int* d_split, int n_rir, const void* d_table, size_t table_bytes,
                             const gtcrn_batch_item* d_plan, const gtcrn_reverb_item* d_rplan, int B, long L, short* d_staged,
                             short* d_staged_target, long staged_stride, long long* d_staged_offsets,
                             gtcrn_batch_item* d_staged_plan, gtcrn_reverb_split_record* d_records, void* d_workspace, int form,
                             void* stream) {
    const std::string w("gtcrn_batch_reverb_split");
    gtr::SplitArgs a;
    const int rc = reverb_args(w, d_speech_pcm, d_speech_offsets, n_speech, d_taps, d_rir_offsets, n_rir, d_table, table_bytes,
                               gtr::split_header_bytes(n_rir), d_plan, d_rplan, B, L, d_staged, staged_stride, d_staged_offsets,
                               d_staged_plan, d_records, d_workspace, &form, &a.r);
    if (rc != 0) return rc;
    if (!d_split || !d_staged_target) return rfail(GTCRN_ERR_ARG, w + ": null pointer");
    if ((reinterpret_cast<uintptr_t>(d_split) & 3) || (reinterpret_cast<uintptr_t>(d_staged_target) & 1))
        return rfail(GTCRN_ERR_ARG, w + ": misaligned pointer");
    a.split = d_split;
    a.target = d_staged_target;
    a.srec = reinterpret_cast<gtr::SRecord*>(d_records);
    const int e = gtr::launch_split(a, form, static_cast<hipStream_t>(stream));
    if (e != 0) return rfail(GTCRN_ERR_HIP, w + ": " + hipGetErrorString(static_cast<hipError_t>(e)));
    return 0;
}

int gtcrn_selftest_mfma_i8(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return rfail(GTCRN_ERR_DEVICE, "no HIP device");
    DeviceScope restore;
    if (hipSetDevice(device) != hipSuccess) return rfail(GTCRN_ERR_DEVICE, "gtcrn_selftest_mfma_i8: no such device");
    signed char hA[16 * 64], hB[64 * 16];
    int hC[256], hD[256], ref[256];
    for (int i = 0; i < 16; ++i)
        for (int k = 0; k < 64; ++k) hA[i * 64 + k] = (signed char)((i * 37 + k * 11 + (i * k) % 7) % 256 - 128);   // asymmetric, full range
    for (int k = 0; k < 64; ++k)
        for (int j = 0; j < 16; ++j) hB[k * 16 + j] = (signed char)((k * 29 - j * 13 + (j * j) % 5 + 300) % 256 - 128);
    hA[0] = -128; hB[0] = -128; hA[5 * 64 + 63] = 127; hB[63 * 16 + 9] = -128;
    for (int i = 0; i < 256; ++i) hC[i] = (i * 7919) % 200003 - 100000;
    for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j) {
            int s = hC[i * 16 + j];
            for (int k = 0; k < 64; ++k) s += (int)hA[i * 64 + k] * (int)hB[k * 16 + j];
            ref[i * 16 + j] = s;
        }
    DevMem bA, bB, bC, bD;
    if (hipMalloc(&bA.p, sizeof(hA)) != hipSuccess || hipMalloc(&bB.p, sizeof(hB)) != hipSuccess ||
        hipMalloc(&bC.p, sizeof(hC)) != hipSuccess || hipMalloc(&bD.p, sizeof(hD)) != hipSuccess)
        return rfail(GTCRN_ERR_HIP, "gtcrn_selftest_mfma_i8: hipMalloc failed");
    if (hipMemcpy(bA.p, hA, sizeof(hA), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(bB.p, hB, sizeof(hB), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(bC.p, hC, sizeof(hC), hipMemcpyHostToDevice) != hipSuccess)
        return rfail(GTCRN_ERR_HIP, "gtcrn_selftest_mfma_i8: hipMemcpy failed");
    const int e = gtr::launch_selftest_i8(static_cast<const signed char*>(bA.p), static_cast<const signed char*>(bB.p),
                                          static_cast<const int*>(bC.p), static_cast<int*>(bD.p), nullptr);
    if (e != 0) return rfail(GTCRN_ERR_HIP, std::string("gtcrn_selftest_mfma_i8: ") + hipGetErrorString(static_cast<hipError_t>(e)));
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(hD, bD.p, sizeof(hD), hipMemcpyDeviceToHost) != hipSuccess)
        return rfail(GTCRN_ERR_HIP, "gtcrn_selftest_mfma_i8: the kernel or the copy back failed");
    int bad = 0;
    for (int i = 0; i < 256; ++i) bad += hD[i] != ref[i];
    if (bad) return rfail(GTCRN_ERR_DEVICE, "MFMA 16x16x64 i8 lane map differs from the assumed one (" + std::to_string(bad) +
                                                " of 256 elements)");
    return 0;
}
