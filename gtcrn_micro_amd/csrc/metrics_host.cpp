// metrics_host.cpp -- the "scores" section of include/gtcrn_micro_hip.h: table design (double, on the host), argument checks
// and launch sequencing.  The arithmetic is in metrics.hip.
#include "../../include/gtcrn_micro_hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "metrics.h"

extern "C" void gtcrn_set_error_(const char* msg);   // api.cpp: thread-local last error
// api.cpp: the resampler section's tap design for any ratio (no rate check); returns 2 half + 1
extern "C" long gtcrn_resample_design_(int fs_in, int fs_out, int* up, int* down, float* h_taps, long cap);

static_assert(sizeof(gtcrn_score_record) == 32 && sizeof(gtm::ScoreRecord) == 32, "the score record is 32 bytes");
static_assert(sizeof(gtcrn_score_ext_record) == 64 && sizeof(gtm::ScoreExtRecord) == 64, "the ext score record is 64 bytes");

namespace {

int sfail(int code, const std::string& m) {
    gtcrn_set_error_(m.c_str());
    return code;
}

constexpr long SC_MAX_L = 1L << 28;       // keeps 8 j + 256 and every frame index inside an int
constexpr int SC_MAX_B = 65535;           // a grid's y extent

void score_window(double* w) {            // w[i] = 0.5 (1 - cos(2 pi (i + 1) / 257))
    const double kPi = 3.14159265358979323846;
    for (int i = 0; i < gtm::SC_FRAME; ++i) w[i] = 0.5 * (1.0 - std::cos(2.0 * kPi * (double)(i + 1) / 257.0));
}

void segsnr_window(double* w) {           // w[i] = 0.5 (1 - cos(2 pi (i + 1) / 481))
    const double kPi = 3.14159265358979323846;
    for (int i = 0; i < gtm::SX_FRAME; ++i) w[i] = 0.5 * (1.0 - std::cos(2.0 * kPi * (double)(i + 1) / 481.0));
}

// nearest bins of 150 * 2^((2 j -/+ 1) / 6) Hz on the grid k * 10000 / 512
void score_band_table(int* lo, int* hi) {
    for (int j = 0; j < gtm::SC_BANDS; ++j) {
        const double fl = 150.0 * std::pow(2.0, (2.0 * j - 1.0) / 6.0), fh = 150.0 * std::pow(2.0, (2.0 * j + 1.0) / 6.0);
        lo[j] = (int)std::floor(fl * 512.0 / 10000.0 + 0.5);
        hi[j] = (int)std::floor(fh * 512.0 / 10000.0 + 0.5);
    }
}

}  // namespace

struct gtcrn_scorer {
    int device = 0;
    char* d_tab = nullptr;                // one allocation: taps, windows, twiddles, band table
    gtm::ScoreTables tab;
    const double* w480 = nullptr;         // the segmental-SNR window, behind the tables
    // the most recent call (test hook)
    char* last_ws = nullptr;
    long last_L = 0;
    int last_B = 0, last_what = 0;
    // stage timing (gtcrn_score_timing)
    bool timing = false;
    hipEvent_t ev[gtm::SC_STAGES + 1] = {};
    hipEvent_t ev_ext[gtm::SX_STAGES + 1] = {};   // ... of gtcrn_score_ext
    bool ev_valid = false;
};

long gtcrn_score_taps(int* up, int* down, float* h_taps, long cap) {
    return gtcrn_resample_design_(16000, 10000, up, down, h_taps, cap);
}

int gtcrn_score_bands(int* lo15, int* hi15) {
    if (!lo15 || !hi15) return sfail(GTCRN_ERR_ARG, "gtcrn_score_bands: null pointer");
    score_band_table(lo15, hi15);
    return 0;
}

long gtcrn_score_frames(long L) {
    if (L < 0 || L > SC_MAX_L) return sfail(GTCRN_ERR_ARG, "gtcrn_score_frames: L outside 0 .. 2^28");
    return gtm::score_frames_of(gtm::score_n10(L));
}

size_t gtcrn_score_workspace_bytes(int B, long L) {
    if (B < 1 || B > SC_MAX_B || L < 1 || L > SC_MAX_L) {
        sfail(GTCRN_ERR_ARG, "gtcrn_score_workspace_bytes: B outside 1 .. 65535 or L outside 1 .. 2^28");
        return 0;
    }
    return (size_t)B * (size_t)gtm::score_layout(L).clip_bytes;
}

int gtcrn_scorer_create(gtcrn_scorer** out, int device) {
    if (!out) return sfail(GTCRN_ERR_ARG, "gtcrn_scorer_create: null out pointer");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return sfail(GTCRN_ERR_DEVICE, "no HIP device");
    if (device < 0 || device >= ndev) return sfail(GTCRN_ERR_ARG, "gtcrn_scorer_create: no such device");
    // host image of the tables, every part at a multiple of 16 bytes
    const size_t o_taps = 0, o_win = 2112, o_winf = o_win + 256 * 8, o_tw256 = o_winf + 256 * 4, o_tw512 = o_tw256 + 256 * 8,
                 o_bands = o_tw512 + 256 * 8, o_w480 = o_bands + 128, total = o_w480 + gtm::SX_FRAME * 8;
    std::vector<char> img(total, 0);
    int up = 0, down = 0;
    if (gtcrn_score_taps(&up, &down, reinterpret_cast<float*>(img.data() + o_taps), gtm::SC_NTAPS) != gtm::SC_NTAPS ||
        up != gtm::SC_UP || down != gtm::SC_DOWN)
        return sfail(GTCRN_ERR_STATE, "gtcrn_scorer_create: the 5/8 stage's design is not 513 taps");
    double* w = reinterpret_cast<double*>(img.data() + o_win);
    float* wf = reinterpret_cast<float*>(img.data() + o_winf);
    score_window(w);
    for (int i = 0; i < gtm::SC_FRAME; ++i) wf[i] = (float)w[i];
    const double kPi = 3.14159265358979323846;
    float* t256 = reinterpret_cast<float*>(img.data() + o_tw256);
    float* t512 = reinterpret_cast<float*>(img.data() + o_tw512);
    for (int k = 0; k < 256; ++k) {
        t256[2 * k] = (float)std::cos(2.0 * kPi * k / 256.0); t256[2 * k + 1] = (float)-std::sin(2.0 * kPi * k / 256.0);
        t512[2 * k] = (float)std::cos(2.0 * kPi * k / 512.0); t512[2 * k + 1] = (float)-std::sin(2.0 * kPi * k / 512.0);
    }
    int* bands = reinterpret_cast<int*>(img.data() + o_bands);
    score_band_table(bands, bands + gtm::SC_BANDS);
    segsnr_window(reinterpret_cast<double*>(img.data() + o_w480));
    gtcrn_scorer* s = new gtcrn_scorer;
    s->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->d_tab), total);
    if (e == hipSuccess) e = hipMemcpy(s->d_tab, img.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (s->d_tab) (void)hipFree(s->d_tab);
        delete s;
        return sfail(GTCRN_ERR_HIP, std::string("gtcrn_scorer_create: ") + hipGetErrorString(e));
    }
    s->tab.taps = reinterpret_cast<const float*>(s->d_tab + o_taps);
    s->tab.win = reinterpret_cast<const double*>(s->d_tab + o_win);
    s->tab.winf = reinterpret_cast<const float*>(s->d_tab + o_winf);
    s->tab.tw256 = reinterpret_cast<const float2*>(s->d_tab + o_tw256);
    s->tab.tw512 = reinterpret_cast<const float2*>(s->d_tab + o_tw512);
    s->tab.bands = reinterpret_cast<const int*>(s->d_tab + o_bands);
    s->w480 = reinterpret_cast<const double*>(s->d_tab + o_w480);
    *out = s;
    return 0;
}

void gtcrn_scorer_destroy(gtcrn_scorer* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    if (s->ev_valid) {
        for (hipEvent_t e : s->ev) (void)hipEventDestroy(e);
        for (hipEvent_t e : s->ev_ext) (void)hipEventDestroy(e);
    }
    if (s->d_tab) (void)hipFree(s->d_tab);
    delete s;
}

int gtcrn_score(gtcrn_scorer* s, const float* d_ref, long ref_stride, const float* d_inf, long inf_stride, const int* d_lengths,
                long L, int B, int what, gtcrn_score_record* d_out, void* d_workspace, void* stream) {
    const std::string w("gtcrn_score");
    if (!s || !s->d_tab) return sfail(GTCRN_ERR_ARG, w + ": null scorer");
    if (!d_ref || !d_inf || !d_out) return sfail(GTCRN_ERR_ARG, w + ": null pointer");
    if (B < 1 || B > SC_MAX_B || L < 1 || L > SC_MAX_L) return sfail(GTCRN_ERR_ARG, w + ": B outside 1 .. 65535 or L outside 1 .. 2^28");
    if (ref_stride < L || inf_stride < L) return sfail(GTCRN_ERR_ARG, w + ": a stride is shorter than its row");
    if (what < 1 || what > 7) return sfail(GTCRN_ERR_ARG, w + ": `what` is a sum of 1 (SDR), 2 (SI-SNR) and 4 (STOI)");
    if ((what & 4) && (!d_workspace || (reinterpret_cast<uintptr_t>(d_workspace) & 15)))
        return sfail(GTCRN_ERR_ARG, w + ": STOI needs a 16-byte aligned workspace of gtcrn_score_workspace_bytes(B, L)");
    if (reinterpret_cast<uintptr_t>(d_out) & 7) return sfail(GTCRN_ERR_ARG, w + ": d_out must be 8-byte aligned");
    gtm::ScorePlan p;
    p.ref = d_ref; p.inf = d_inf; p.ref_stride = ref_stride; p.inf_stride = inf_stride;
    p.lens = d_lengths; p.L = L; p.B = B; p.what = what;
    p.out = reinterpret_cast<gtm::ScoreRecord*>(d_out);
    p.ws = static_cast<char*>(d_workspace);
    p.lay = gtm::score_layout(L);
    p.tab = s->tab;
    hipError_t e = hipSetDevice(s->device);
    if (e != hipSuccess) return sfail(GTCRN_ERR_HIP, w + ": " + hipGetErrorString(e));
    const int rc = gtm::launch_score(p, static_cast<hipStream_t>(stream), s->timing ? s->ev : nullptr);
    if (rc != 0) return sfail(GTCRN_ERR_HIP, w + ": " + hipGetErrorString(static_cast<hipError_t>(rc)));
    s->last_ws = (what & 4) ? p.ws : nullptr;
    s->last_L = L; s->last_B = B; s->last_what = what;
    return 0;
}

long gtcrn_score_debug(gtcrn_scorer* s, int which, int b, float* d_dst, long cap, void* stream) {
    const std::string w("gtcrn_score_debug");
    if (!s || !s->d_tab) return sfail(GTCRN_ERR_ARG, w + ": null scorer");
    if (!s->last_ws) return sfail(GTCRN_ERR_STATE, w + ": no call with STOI came before");
    if (which < 0 || which > 4 || b < 0 || b >= s->last_B || !d_dst) return sfail(GTCRN_ERR_ARG, w + ": bad `which`, row or destination");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipSetDevice(s->device);
    const gtm::ScoreLayout lay = gtm::score_layout(s->last_L);
    const char* ws = s->last_ws + (long)b * lay.clip_bytes;
    int h[gtm::SC_H_WORDS] = {};
    if (e == hipSuccess) e = hipMemcpyAsync(h, ws, sizeof(h), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return sfail(GTCRN_ERR_HIP, w + ": " + hipGetErrorString(e));
    const long n10 = h[gtm::SC_H_N10], nfr = h[gtm::SC_H_NFR], M = h[gtm::SC_H_M];
    if (n10 < 0 || n10 > lay.n10 || nfr < 0 || nfr > lay.nfr || M < 0 || M >= (nfr > 0 ? nfr : 1))
        return sfail(GTCRN_ERR_STATE, w + ": the workspace does not hold the most recent call's header");
    const long n = which == 0 ? n10 : which <= 2 ? nfr : (long)gtm::SC_BANDS * M;
    if (cap < n) return sfail(GTCRN_ERR_ARG, w + ": the destination holds fewer floats than the result");
    if (n == 0) return 0;
    int rc = 0;
    if (which == 0) e = hipMemcpyAsync(d_dst, ws + lay.o_x10, sizeof(float) * n, hipMemcpyDeviceToDevice, st);
    else if (which == 1) rc = gtm::launch_score_debug_cvt(ws + lay.o_edb, 0, d_dst, n, st);
    else if (which == 2) rc = gtm::launch_score_debug_cvt(ws + lay.o_flag, 1, d_dst, n, st);
    else
        e = hipMemcpy2DAsync(d_dst, sizeof(float) * M, ws + lay.o_env + (which == 4 ? sizeof(float) * gtm::SC_BANDS * lay.env_stride : 0),
                             sizeof(float) * lay.env_stride, sizeof(float) * M, gtm::SC_BANDS, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess || rc != 0)
        return sfail(GTCRN_ERR_HIP, w + ": " + hipGetErrorString(e != hipSuccess ? e : static_cast<hipError_t>(rc)));
    return n;
}

int gtcrn_score_timing(gtcrn_scorer* s, int on) {
    if (!s) return sfail(GTCRN_ERR_ARG, "gtcrn_score_timing: null scorer");
    if (on && !s->ev_valid) {
        hipError_t e = hipSetDevice(s->device);
        for (hipEvent_t& ev : s->ev)
            if (e == hipSuccess) e = hipEventCreate(&ev);
        for (hipEvent_t& ev : s->ev_ext)
            if (e == hipSuccess) e = hipEventCreate(&ev);
        if (e != hipSuccess) return sfail(GTCRN_ERR_HIP, std::string("gtcrn_score_timing: ") + hipGetErrorString(e));
        s->ev_valid = true;
    }
    s->timing = on != 0;
    return 0;
}

int gtcrn_score_timing_read(gtcrn_scorer* s, int stage, char* name, int name_cap, float* ms) {
    if (!s || !ms || stage < 0 || stage >= gtm::SC_STAGES) return sfail(GTCRN_ERR_ARG, "gtcrn_score_timing_read: bad argument");
    if (!s->ev_valid) return sfail(GTCRN_ERR_STATE, "gtcrn_score_timing_read: timing was never enabled");
    hipError_t e = hipEventSynchronize(s->ev[gtm::SC_STAGES]);
    if (e == hipSuccess) e = hipEventElapsedTime(ms, s->ev[stage], s->ev[stage + 1]);
    if (e != hipSuccess) return sfail(GTCRN_ERR_HIP, std::string("gtcrn_score_timing_read: ") + hipGetErrorString(e));
    if (name && name_cap > 0) {
        std::strncpy(name, gtm::score_stage_name(stage), (size_t)name_cap - 1);
        name[name_cap - 1] = 0;
    }
    return 0;
}

// ---- gtcrn_score_ext: the three scores above plus ESTOI and segmental SNR, 64-byte records

long gtcrn_score_segsnr_frames(long n) {
    if (n < 0 || n > SC_MAX_L) return sfail(GTCRN_ERR_ARG, "gtcrn_score_segsnr_frames: n outside 0 .. 2^28");
    return gtm::score_segsnr_frames_of(n);
}

int gtcrn_score_segsnr_window(double* h_w480) {
    if (!h_w480) return sfail(GTCRN_ERR_ARG, "gtcrn_score_segsnr_window: null pointer");
    segsnr_window(h_w480);
    return 0;
}

size_t gtcrn_score_ext_workspace_bytes(int B, long L) {
    if (B < 1 || B > SC_MAX_B || L < 1 || L > SC_MAX_L) {
        sfail(GTCRN_ERR_ARG, "gtcrn_score_ext_workspace_bytes: B outside 1 .. 65535 or L outside 1 .. 2^28");
        return 0;
    }
    return gtm::score_ext_bytes(B, L);
}

int gtcrn_score_ext(gtcrn_scorer* s, const float* d_ref, long ref_stride, const float* d_inf, long inf_stride, const int* d_lengths,
                    long L, int B, int what, gtcrn_score_ext_record* d_out, void* d_workspace, void* stream) {
    const std::string w("gtcrn_score_ext");
    if (!s || !s->d_tab) return sfail(GTCRN_ERR_ARG, w + ": null scorer");
    if (!d_ref || !d_inf || !d_out) return sfail(GTCRN_ERR_ARG, w + ": null pointer");
    if (B < 1 || B > SC_MAX_B || L < 1 || L > SC_MAX_L) return sfail(GTCRN_ERR_ARG, w + ": B outside 1 .. 65535 or L outside 1 .. 2^28");
    if (ref_stride < L || inf_stride < L) return sfail(GTCRN_ERR_ARG, w + ": a stride is shorter than its row");
    if (what < 1 || what > 31)
        return sfail(GTCRN_ERR_ARG, w + ": `what` is a sum of 1 (SDR), 2 (SI-SNR), 4 (STOI), 8 (ESTOI) and 16 (segmental SNR)");
    if ((what & 28) && (!d_workspace || (reinterpret_cast<uintptr_t>(d_workspace) & 15)))
        return sfail(GTCRN_ERR_ARG, w + ": STOI, ESTOI and segmental SNR need a 16-byte aligned workspace of gtcrn_score_ext_workspace_bytes(B, L)");
    if (reinterpret_cast<uintptr_t>(d_out) & 7) return sfail(GTCRN_ERR_ARG, w + ": d_out must be 8-byte aligned");
    gtm::ScoreExtPlan x = gtm::score_ext_layout(L);
    gtm::ScorePlan& p = x.base;
    p.ref = d_ref; p.inf = d_inf; p.ref_stride = ref_stride; p.inf_stride = inf_stride;
    p.lens = d_lengths; p.L = L; p.B = B; p.what = what & 7;
    p.out = static_cast<gtm::ScoreRecord*>(d_workspace);                          // B records, then the B slices
    p.ws = d_workspace ? static_cast<char*>(d_workspace) + (size_t)B * sizeof(gtm::ScoreRecord) : nullptr;
    p.tab = s->tab;
    x.what = what;
    x.w480 = s->w480;
    x.out = reinterpret_cast<gtm::ScoreExtRecord*>(d_out);
    hipError_t e = hipSetDevice(s->device);
    if (e != hipSuccess) return sfail(GTCRN_ERR_HIP, w + ": " + hipGetErrorString(e));
    const int rc = gtm::launch_score_ext(x, static_cast<hipStream_t>(stream), s->timing ? s->ev_ext : nullptr);
    if (rc != 0) return sfail(GTCRN_ERR_HIP, w + ": " + hipGetErrorString(static_cast<hipError_t>(rc)));
    return 0;
}

int gtcrn_score_ext_stages(void) { return gtm::SX_STAGES; }

int gtcrn_score_ext_timing_read(gtcrn_scorer* s, int stage, char* name, int name_cap, float* ms) {
    if (!s || !ms || stage < 0 || stage >= gtm::SX_STAGES) return sfail(GTCRN_ERR_ARG, "gtcrn_score_ext_timing_read: bad argument");
    if (!s->ev_valid) return sfail(GTCRN_ERR_STATE, "gtcrn_score_ext_timing_read: timing was never enabled");
    hipError_t e = hipEventSynchronize(s->ev_ext[gtm::SX_STAGES]);
    if (e == hipSuccess) e = hipEventElapsedTime(ms, s->ev_ext[stage], s->ev_ext[stage + 1]);
    if (e != hipSuccess) return sfail(GTCRN_ERR_HIP, std::string("gtcrn_score_ext_timing_read: ") + hipGetErrorString(e));
    if (name && name_cap > 0) {
        std::strncpy(name, gtm::score_ext_stage_name(stage), (size_t)name_cap - 1);
        name[name_cap - 1] = 0;
    }
    return 0;
}
