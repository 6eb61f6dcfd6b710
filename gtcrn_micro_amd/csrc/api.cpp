// api.cpp -- the C ABI of include/gtcrn_micro_hip.h: handle, workspace, launch sequencing.
// Host code only; every arithmetic step runs in kernels.hip on the GPU.  There is no CPU fallback:
// without a gfx950 device gtcrn_model_create fails.
#include "../../include/gtcrn_micro_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "kernels.h"
#include "layout.h"
#include "pack.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int hip_fail(hipError_t e, const char* what) {
    return fail(GTCRN_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(expr)                                         \
    do {                                                      \
        hipError_t e_ = (expr);                               \
        if (e_ != hipSuccess) return hip_fail(e_, #expr);     \
    } while (0)
#define LAUNCH_TRY(expr)                                                         \
    do {                                                                         \
        int e_ = (expr);                                                         \
        if (e_ != 0) return hip_fail(static_cast<hipError_t>(e_), #expr);        \
    } while (0)

// HIP-event timing of every kernel launch, kept per call so that a whole timed region can be
// averaged afterwards without synchronising inside it.
struct Timing {
    int kernel = 0;  // index into kKernelNames
    hipEvent_t a = nullptr, b = nullptr;
};
// every timed launch records WHICH kernel it was (mixed offline / streaming calls keep their own rows).  The order is ABI:
// gtcrn_timing_enable(m, 2 + k) and gtcrn_timing_read address a kernel by its index, so new rows go at the end.
#define GT_KERNELS(X)                                                                                                     \
    X(K_STFT, "k_stft") X(K_ENCODER, "k_encoder") X(K_GTCN1, "k_gtcn1") X(K_GTCN2, "k_gtcn2") X(K_DECODER, "k_decoder")   \
    X(K_ISTFT, "k_istft") X(K_FRONT, "k_front") X(K_ENCODER_GT, "k_encoder_gt") X(K_GTCN_MS, "k_gtcn_ms")                 \
    X(K_STREAM_MS, "k_stream_ms") X(K_STREAM_WIDE, "k_stream_wide") X(K_WAVE_ANALYSIS, "k_wave_analysis")                 \
    X(K_WAVE_SYNTHESIS, "k_wave_synthesis") X(K_PACKET_IN, "k_packet_in") X(K_PACKET_OUT, "k_packet_out")                 \
    X(K_WAVE_SYNTHESIS_MIX, "k_wave_synthesis_mix") X(K_ISTFT_MIX, "k_istft_mix") X(K_PACKET_PLAN, "k_packet_plan")       \
    X(K_PACKET_IN_SLOTS, "k_packet_in_slots") X(K_PACKET_OUT_SLOTS, "k_packet_out_slots")                                 \
    X(K_WAVE_SYNTHESIS_METER, "k_wave_synthesis_meter")
#define GT_KERNEL_ID(id, name) id,
#define GT_KERNEL_NAME(id, name) name,
enum KernelId { GT_KERNELS(GT_KERNEL_ID) K_COUNT };
const char* const kKernelNames[K_COUNT] = {GT_KERNELS(GT_KERNEL_NAME)};
constexpr int kNumKernels = K_COUNT;

}  // namespace

// train.cpp reports its errors through the same thread-local message
extern "C" void gtcrn_set_error_(const char* msg) { g_err = msg ? msg : ""; }

struct gtcrn_model {
    int device = 0;
    float* d_pf = nullptr;   // packed floats (gtl::P_FLOATS)
    float* d_pfq = nullptr;  // the same with int8-quantised weights (BASELINE configs[4] variant)
    int* d_pi = nullptr;     // packed ints (gtl::P_INTS)
    float* d_twid = nullptr; // 512 complex twiddles
    int* d_pref = nullptr;   // prefix table of a variable-length batch (1025 ints, see gtk::launch_len_prefix)
    bool var_spans = true;   // variable-length batches run in time spans (off: one workgroup per utterance, the A/B switch)
    int stream_form = 0;     // single-frame streaming steps: 0 = ONE launch, the form picked by the stream count (four
                             // streams per workgroup, k_stream_ms, or seven, k_stream_wide: stream_wide_pays); 1 = the
                             // three-launch form (encoder / both GTCN stacks / decoder, hand-offs through HBM); 2 / 3 =
                             // ONE launch, k_stream_ms / k_stream_wide whatever the count: the A/B switches
    std::vector<int> h_pi;   // host copy of the int tables (slot permutations for the debug taps)
    // workspace for B x T
    long cap_bt = 0;         // capacity in (batch * frames)
    int last_B = 0, last_T = 0;
    float* d_en0 = nullptr;  // (B,T,65,16)
    float* d_en[4] = {nullptr, nullptr, nullptr, nullptr};  // en1..en4 (B,T,33,16)
    float* d_g1 = nullptr;   // gtcn1 output
    float* d_g2 = nullptr;   // gtcn2 output
    float* d_spec_a = nullptr;  // frame-major spectrograms for forward_wave (B,T,257,2)
    float* d_spec_b = nullptr;
    float* d_rate_a = nullptr;  // 16 kHz hand-offs of gtcrn_rate_stream_step (nstreams x 256 nhops each): k_rate_in -> wave step,
    float* d_rate_b = nullptr;  // wave step -> k_rate_out; sized by gtcrn_rate_stream_reserve
    gtk::WaveOpts live;         // the caller's buffers of gtcrn_wave_stream_set_meters / _gain_ramp / _alc (gain: per call)
    long cap_rate = 0;          // capacity of each in (streams * hops)
    bool debug = false;
    bool debug_keep_fused = false;   // gtcrn_debug_enable(m, 2): phase stamps only -- single-frame steps stay ONE launch
    float* d_dbg = nullptr;
    long dbg_cap_bt = 0;
    unsigned long long* d_stamps = nullptr;  // [4 kernels][B][16] phase cycle sums (diagnostic build only)
    int stamps_cap_b = 0;
    float** d_ptr8 = nullptr;  // device table of 8 tcn cache pointers
    bool last_quant = false;       // the last forward was the fp16 variant: the hand-off buffers hold fp16 records
    bool last_quant_taps = false;  // ... and ran with the stage taps enabled (gtcrn_debug_enable 1): gtcrn_debug_tap serves it
    bool last_fused_stream = false;  // the last forward was the single-launch streaming step: no hand-off tensors exist
    bool timing = false;
    int timing_only = -1;          // >= 0: record events around this kernel only (two events per call)
    std::vector<Timing> timings;   // one entry per timed launch since gtcrn_timing_enable(m, 1)
    std::vector<Timing> ev_pool;   // recycled events
};

namespace {

void free_workspace(gtcrn_model* m) {
    float** bufs[] = {&m->d_en0, &m->d_en[0], &m->d_en[1], &m->d_en[2], &m->d_en[3], &m->d_g1, &m->d_g2,
                      &m->d_spec_a, &m->d_spec_b};
    for (float** p : bufs) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    m->cap_bt = 0;
}

// A buffer has to grow: refused while `s` is being captured (`what` says which reserve call was missing), otherwise the
// device is drained so that the caller may free and allocate.
int before_growing(hipStream_t s, const char* what) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return fail(GTCRN_ERR_STATE, what);
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}

// every state buffer of the live calls is read and written with 16-byte accesses
int check_state_alignment(const std::string& w, std::initializer_list<const void*> states) {
    uintptr_t bits = 0;
    for (const void* p : states) bits |= reinterpret_cast<uintptr_t>(p);
    if (bits & 15) return fail(GTCRN_ERR_ARG, w + ": the state buffers must be 16-byte aligned");
    return 0;
}

int ensure_workspace(gtcrn_model* m, int B, int T, hipStream_t s) {
    const long bt = (long)B * T;
    if (bt > m->cap_bt) {
        if (int rc = before_growing(s, "workspace too small during stream capture: call gtcrn_model_reserve first")) return rc;
        free_workspace(m);
        HIP_TRY(hipMalloc(&m->d_en0, sizeof(float) * bt * 65 * 16));
        for (int i = 0; i < 4; ++i) HIP_TRY(hipMalloc(&m->d_en[i], sizeof(float) * bt * 528));
        HIP_TRY(hipMalloc(&m->d_g1, sizeof(float) * bt * 528));
        HIP_TRY(hipMalloc(&m->d_g2, sizeof(float) * bt * 528));
        HIP_TRY(hipMalloc(&m->d_spec_a, sizeof(float) * bt * 514));
        HIP_TRY(hipMalloc(&m->d_spec_b, sizeof(float) * bt * 514));
        m->cap_bt = bt;
    }
    if (m->debug && bt > m->dbg_cap_bt) {
        if (m->d_dbg) (void)hipFree(m->d_dbg);
        m->d_dbg = nullptr;
        HIP_TRY(hipMalloc(&m->d_dbg, sizeof(float) * bt * (3 * 528 + 65 * 16 + 2 * 129)));
        m->dbg_cap_bt = bt;
    }
    if (m->debug && B + 2048 > m->stamps_cap_b) {
        // one row per WORKGROUP: launches in time spans run up to 2048 of them whatever the batch
        const int rows = B + 2048;        // (a split plan: nA <= B one-per-utterance rows, then up to 2048 share rows behind them)
        if (m->d_stamps) (void)hipFree(m->d_stamps);
        m->d_stamps = nullptr;
        HIP_TRY(hipMalloc(&m->d_stamps, sizeof(unsigned long long) * 4 * rows * 16));
        HIP_TRY(hipMemset(m->d_stamps, 0, sizeof(unsigned long long) * 4 * rows * 16));
        m->stamps_cap_b = rows;
    }
    return 0;
}

struct Timer {
    gtcrn_model* m;
    hipStream_t s;
    Timer(gtcrn_model* m_, hipStream_t s_) : m(m_), s(s_) {}
    bool on = false;
    void begin(int kernel) {
        on = m->timing && (m->timing_only < 0 || m->timing_only == kernel);
        if (!on) return;
        Timing t;
        if (!m->ev_pool.empty()) {
            t = m->ev_pool.back();
            m->ev_pool.pop_back();
        } else {
            (void)hipEventCreate(&t.a);
            (void)hipEventCreate(&t.b);
        }
        t.kernel = kernel;
        (void)hipEventRecord(t.a, s);
        m->timings.push_back(t);
    }
    void end() {
        if (!on) return;
        (void)hipEventRecord(m->timings.back().b, s);
    }
};

// Single-frame steps of B streams: k_stream_ms serves four streams per workgroup, k_stream_wide seven in a workgroup that
// takes WIDE_COST times as long (measured: profiles/r06_ab_stream_wide.txt).  Both run one workgroup per CU, so a step
// costs rounds-of-256-workgroups x the form's time: the wide form pays once the narrow one needs more rounds than it.
static bool stream_wide_pays(int B) {
    constexpr double WIDE_COST = 1.5;      // 49.3 us against 32.9 us per round of 256 workgroups at 65 536 streams
    const int ws = gtk::stream_wide_streams();
    const long r4 = ((B + 3) / 4 + 255) / 256, r7 = ((B + ws - 1) / ws + 255) / 256;
    return (double)r7 * WIDE_COST < (double)r4;
}

// Single-frame steps run as ONE launch, nothing handed over through HBM, unless the three-launch form is asked for
// (gtcrn_stream_form 1, or the stage taps of the parity tests, which read the hand-off tensors).
bool fused_stream_allowed(const gtcrn_model* m) { return (!m->debug || m->debug_keep_fused) && m->stream_form != 1; }

// The single-launch step of B streams (rows.slots: of the max_active = B rows the table names): picks the form, brackets the
// launch for the timing rows and records what the last forward was.  The caller has checked fused_stream_allowed and
// gtk::stream_ms_usable.
int fused_stream_step(gtcrn_model* m, const float* spec_in, long isb, long isf, float* spec_out, long osb, long osf, int B,
                      float* state, gtk::Rows rows, hipStream_t s) {
    const bool wide = m->stream_form == 3 || (m->stream_form == 0 && stream_wide_pays(B));
    unsigned long long* stamps = (m->debug && m->d_stamps) ? m->d_stamps : nullptr;
    Timer tm(m, s);
    tm.begin(wide ? K_STREAM_WIDE : K_STREAM_MS);
    LAUNCH_TRY(gtk::launch_stream_step(wide, spec_in, isb, isf, spec_out, osb, osf, B, m->d_pf, m->d_pi, state, stamps, rows, s));
    tm.end();
    m->last_quant = false;
    m->last_fused_stream = true;
    m->last_B = B;
    m->last_T = 1;
    return 0;
}

// the five model kernels on one stream; state == nullptr for offline
int run_model(gtcrn_model* m, const float* spec_in, long isb, long isf, long ist, float* spec_out, long osb, long osf,
              long ost, int B, int T, float* state, hipStream_t s, const int* lens = nullptr,
              const gtk::Quant* q = nullptr, bool front_done = false) {
    if (state && T == 1 && !q && fused_stream_allowed(m) && gtk::stream_ms_usable(isb, osb))
        return fused_stream_step(m, spec_in, isb, isf, spec_out, osb, osf, B, state, gtk::Rows{}, s);
    Timer tm(m, s);
    const float* pf = q ? m->d_pfq : m->d_pf;
    const bool offline = !state;
    m->last_quant = q != nullptr;
    m->last_quant_taps = q != nullptr && m->debug;
    m->last_fused_stream = false;
    if (offline) {
        // offline: the frame-independent front end runs as a throughput kernel (fused with the STFT by
        // forward_wave_impl, which passes front_done), the per-utterance kernel keeps the three GTConv blocks
        if (!front_done) {
            tm.begin(K_FRONT);
            LAUNCH_TRY(gtk::launch_front(nullptr, 0, spec_in, isb, isf, ist, B, T, lens, nullptr, nullptr, pf, m->d_pi,
                                         nullptr, m->d_en0, m->d_en[0], s, q));
            tm.end();
        }
    }
    // variable-length offline batches: the per-utterance kernels share the frames that exist (time spans over a prefix
    // table of the lengths) -- unless the batch is whole rounds of the chip already
    const int* pref = nullptr;
    if (offline && lens && !q && front_done && m->var_spans && gtk::var_spans_usable(B) && B % 256 != 0) {
        LAUNCH_TRY(gtk::launch_len_prefix(lens, B, T, m->d_pref, s));
        pref = m->d_pref;
    }
    unsigned long long* stp = (m->debug && m->d_stamps) ? m->d_stamps : nullptr;
    const long sst = (long)m->stamps_cap_b * 16;
    tm.begin(offline ? K_ENCODER_GT : K_ENCODER);
    LAUNCH_TRY(gtk::launch_encoder(spec_in, isb, isf, ist, B, T, lens, pf, m->d_pi, m->d_en0, m->d_en[0], m->d_en[1],
                                   m->d_en[2], m->d_en[3], state, stp ? stp : nullptr, s, q, offline, pref));
    tm.end();
    // GTCN: offline calls (no stream state) use the frequency-band form (registers + wave-private LDS, no barrier);
    // single-frame streaming steps run BOTH stacks per position in one launch; other streaming chunkings use the
    // ring form, whose chunks may hold any number of frames
    if (state && T == 1) {
        tm.begin(K_GTCN_MS);
        LAUNCH_TRY(gtk::launch_gtcn_ms(m->d_en[3], m->d_g1, m->d_g2, pf + gtl::P_GTCN, B, state, s));
        tm.end();
    } else {
        tm.begin(K_GTCN1);
        if (!state)
            LAUNCH_TRY(gtk::launch_gtcn_band(m->d_en[3], m->d_g1, pf + gtl::P_GTCN, B, T, lens, nullptr, s, q, pref));
        else
            LAUNCH_TRY(gtk::launch_gtcn(m->d_en[3], m->d_g1, pf + gtl::P_GTCN, B, T, state, gtk::ST_G1_H, nullptr,
                                        stp ? stp + sst : nullptr, s));
        tm.end();
        tm.begin(K_GTCN2);
        // the second stack stores gtcn2(x) + en_outs[4]: exactly the decoder's first input (Decoder.forward :467)
        if (!state)
            LAUNCH_TRY(gtk::launch_gtcn_band(m->d_g1, m->d_g2, pf + gtl::P_GTCN + gtl::GTCN_SIZE, B, T, lens, m->d_en[3], s,
                                             q, pref));
        else
            LAUNCH_TRY(gtk::launch_gtcn(m->d_g1, m->d_g2, pf + gtl::P_GTCN + gtl::GTCN_SIZE, B, T, state, gtk::ST_G2_H,
                                        m->d_en[3], stp ? stp + 2 * sst : nullptr, s));
        tm.end();
    }
    tm.begin(K_DECODER);
    LAUNCH_TRY(gtk::launch_decoder(m->d_g2, m->d_en0, m->d_en[0], m->d_en[1], m->d_en[2], m->d_en[3], spec_in, isb, isf,
                                   ist, spec_out, osb, osf, ost, B, T, lens, pf, m->d_pi, state,
                                   m->debug ? m->d_dbg : nullptr, stp ? stp + 3 * sst : nullptr, s, q, pref));
    tm.end();
    m->last_B = B;
    m->last_T = T;
    return 0;
}

// 256 complex twiddles of the 256-point FFT, then 256 of the real split's 512-point ones
void make_twiddles(std::vector<float>& tw) {
    tw.resize(1024);
    for (int k = 0; k < 256; ++k) {
        tw[2 * k] = (float)std::cos(-2.0 * M_PI * k / 256.0);
        tw[2 * k + 1] = (float)std::sin(-2.0 * M_PI * k / 256.0);
        tw[512 + 2 * k] = (float)std::cos(-2.0 * M_PI * k / 512.0);
        tw[512 + 2 * k + 1] = (float)std::sin(-2.0 * M_PI * k / 512.0);
    }
}

int check_model(gtcrn_model* m) {
    if (!m || !m->d_pf) return fail(GTCRN_ERR_STATE, "invalid model handle");
    HIP_TRY(hipSetDevice(m->device));
    return 0;
}

int upload_params(gtcrn_model* m, const float* h_params, long n) {
    std::vector<float> F(gtl::P_FLOATS);
    std::vector<int> I(gtl::P_INTS);
    std::string err;
    if (gtcrn::pack_params(h_params, n, F.data(), I.data(), err) != 0) return fail(GTCRN_ERR_ARG, err);
    HIP_TRY(hipMemcpy(m->d_pf, F.data(), sizeof(float) * gtl::P_FLOATS, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->d_pi, I.data(), sizeof(int) * gtl::P_INTS, hipMemcpyHostToDevice));
    gtcrn::quantize_packed(F.data());
    HIP_TRY(hipMemcpy(m->d_pfq, F.data(), sizeof(float) * gtl::P_FLOATS, hipMemcpyHostToDevice));
    m->h_pi = I;
    return 0;
}

}  // namespace

extern "C" {

int gtcrn_abi_version(void) { return GTCRN_ABI_VERSION; }
const char* gtcrn_last_error(void) { return g_err.c_str(); }

long gtcrn_param_tensors(void) { return (long)gtcrn::param_table().size(); }
const char* gtcrn_param_name(long i) {
    const auto& t = gtcrn::param_table();
    return (i < 0 || i >= (long)t.size()) ? nullptr : t[i].name.c_str();
}
long gtcrn_param_numel(long i) {
    const auto& t = gtcrn::param_table();
    return (i < 0 || i >= (long)t.size()) ? -1 : t[i].numel;
}
long gtcrn_param_offset(long i) {
    const auto& t = gtcrn::param_table();
    return (i < 0 || i >= (long)t.size()) ? -1 : t[i].offset;
}

// Host-only view of the packer for the CPU test-suite (no device needed): fills the slot-space
// buffers the kernels consume.  Sizes: gtcrn_pack_sizes().
void gtcrn_pack_sizes(long* n_floats, long* n_ints) {
    if (n_floats) *n_floats = gtl::P_FLOATS;
    if (n_ints) *n_ints = gtl::P_INTS;
}
int gtcrn_pack_params_host(const float* h_params, long n, float* h_f, int* h_i) {
    std::string err;
    if (gtcrn::pack_params(h_params, n, h_f, h_i, err) != 0) return fail(GTCRN_ERR_ARG, err);
    return 0;
}
int gtcrn_pack_params_quant_host(const float* h_params, long n, float* h_f, int* h_i) {
    int rc = gtcrn_pack_params_host(h_params, n, h_f, h_i);
    if (rc == 0) gtcrn::quantize_packed(h_f);
    return rc;
}
float gtcrn_round_to_half(float x) { return gtcrn::round_to_half(x); }

int gtcrn_model_create(gtcrn_model** out, const float* h_params, long n_floats, int device) {
    if (!out || !h_params) return fail(GTCRN_ERR_ARG, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(GTCRN_ERR_DEVICE, "no HIP device: this library has no CPU path");
    if (device < 0 || device >= ndev) return fail(GTCRN_ERR_ARG, "device ordinal out of range");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(GTCRN_ERR_DEVICE, std::string("built for gfx950 only, device is ") + prop.gcnArchName);
    HIP_TRY(hipSetDevice(device));
    gtcrn_model* m = new gtcrn_model();
    m->device = device;
    hipError_t e = hipMalloc(&m->d_pf, sizeof(float) * gtl::P_FLOATS);
    if (e == hipSuccess) e = hipMalloc(&m->d_pfq, sizeof(float) * gtl::P_FLOATS);
    if (e == hipSuccess) e = hipMalloc(&m->d_pi, sizeof(int) * gtl::P_INTS);
    if (e == hipSuccess) e = hipMalloc(&m->d_twid, sizeof(float) * 1024);
    if (e == hipSuccess) e = hipMalloc(&m->d_pref, sizeof(int) * 1025);
    if (e == hipSuccess) e = hipMalloc(&m->d_ptr8, sizeof(float*) * 8);
    if (e != hipSuccess) {
        gtcrn_model_destroy(m);
        return hip_fail(e, "hipMalloc(params)");
    }
    std::vector<float> tw;
    make_twiddles(tw);
    e = hipMemcpy(m->d_twid, tw.data(), sizeof(float) * 1024, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        gtcrn_model_destroy(m);
        return hip_fail(e, "hipMemcpy(twiddles)");
    }
    int rc = upload_params(m, h_params, n_floats);
    if (rc == 0) {
        int le = gtk::configure_kernels();
        if (le != 0) rc = hip_fail(static_cast<hipError_t>(le), "hipFuncSetAttribute(dynamic LDS)");
    }
    if (rc != 0) {
        gtcrn_model_destroy(m);
        return rc;
    }
    *out = m;
    return 0;
}

int gtcrn_model_set_params(gtcrn_model* m, const float* h_params, long n_floats) {
    int rc = check_model(m);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return upload_params(m, h_params, n_floats);
}

void gtcrn_model_destroy(gtcrn_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    (void)hipDeviceSynchronize();
    free_workspace(m);
    if (m->d_rate_a) (void)hipFree(m->d_rate_a);
    if (m->d_rate_b) (void)hipFree(m->d_rate_b);
    if (m->d_dbg) (void)hipFree(m->d_dbg);
    if (m->d_stamps) (void)hipFree(m->d_stamps);
    if (m->d_pf) (void)hipFree(m->d_pf);
    if (m->d_pfq) (void)hipFree(m->d_pfq);
    if (m->d_pi) (void)hipFree(m->d_pi);
    if (m->d_twid) (void)hipFree(m->d_twid);
    if (m->d_pref) (void)hipFree(m->d_pref);
    if (m->d_ptr8) (void)hipFree(m->d_ptr8);
    for (auto* v : {&m->timings, &m->ev_pool})
        for (auto& t : *v) {
            if (t.a) (void)hipEventDestroy(t.a);
            if (t.b) (void)hipEventDestroy(t.b);
        }
    delete m;
}

int gtcrn_model_reserve(gtcrn_model* m, int B, int T) {
    int rc = check_model(m);
    if (rc) return rc;
    if (B < 1 || T < 1) return fail(GTCRN_ERR_ARG, "B and T must be >= 1");
    return ensure_workspace(m, B, T, nullptr);
}

int gtcrn_make_window(int kind, float* h_w512) {
    if (!h_w512 || (kind != 0 && kind != 1)) return fail(GTCRN_ERR_ARG, "window kind must be 0 (sqrt-Hann) or 1 (Hann)");
    gtcrn::make_window(kind, h_w512);
    return 0;
}

long gtcrn_num_frames(long L) { return 1 + L / 256; }

// twiddles are per model; the standalone STFT entry points keep one immutable table per device, created once
// under a lock (the only process-wide state of the library; never modified after its creation)
namespace {
float* g_twid[16] = {nullptr};
std::mutex g_twid_mu;
int device_twiddles(float** out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 16) return fail(GTCRN_ERR_DEVICE, "device ordinal >= 16");
    std::lock_guard<std::mutex> lock(g_twid_mu);
    if (!g_twid[dev]) {
        std::vector<float> tw;
        make_twiddles(tw);
        float* d = nullptr;
        HIP_TRY(hipMalloc(&d, sizeof(float) * 1024));
        HIP_TRY(hipMemcpy(d, tw.data(), sizeof(float) * 1024, hipMemcpyHostToDevice));
        g_twid[dev] = d;
    }
    *out = g_twid[dev];
    return 0;
}
}  // namespace

extern "C" int gtcrn_device_twiddles_(float** out) { return device_twiddles(out); }   // for train.cpp

static int check_spec_layout(const void* p, long sb, long sf, long st) {
    // the kernels move the (re, im) pair with 8-byte accesses
    if ((reinterpret_cast<uintptr_t>(p) & 7) || (sb & 1) || (sf & 1) || (st & 1))
        return fail(GTCRN_ERR_ARG, "spectrogram base must be 8-byte aligned and its strides even (re/im pairs)");
    // inside one 16-frame chunk the kernels address with 32-bit element offsets (256 bins, 15 frames)
    const long span = 256 * (sf < 0 ? -sf : sf) + 15 * (st < 0 ? -st : st);
    if (span >= (1L << 31)) return fail(GTCRN_ERR_ARG, "spectrogram strides too large (a chunk must span < 2^31 floats)");
    return 0;
}

int gtcrn_stft(const float* d_wave, int B, long L, const float* d_win, float* d_spec, long sb, long sf, long st,
               void* stream) {
    if (!d_wave || !d_win || !d_spec || B < 1) return fail(GTCRN_ERR_ARG, "null pointer or B < 1");
    if (int rc0 = check_spec_layout(d_spec, sb, sf, st)) return rc0;
    if (L < 257) return fail(GTCRN_ERR_ARG, "reflect padding needs L > 256 samples");
    float* tw = nullptr;
    int rc = device_twiddles(&tw);
    if (rc) return rc;
    LAUNCH_TRY(gtk::launch_stft(d_wave, B, L, (int)gtcrn_num_frames(L), nullptr, d_win, tw, d_spec, sb, sf, st, nullptr,
                                (hipStream_t)stream));
    return 0;
}

int gtcrn_stft_frames(const float* d_wave, int B, long L, const float* d_win, float* d_frames, void* stream) {
    if (!d_wave || !d_win || !d_frames || B < 1) return fail(GTCRN_ERR_ARG, "null pointer or B < 1");
    if (L < 257) return fail(GTCRN_ERR_ARG, "reflect padding needs L > 256 samples");
    float* tw = nullptr;
    int rc = device_twiddles(&tw);
    if (rc) return rc;
    LAUNCH_TRY(gtk::launch_stft(d_wave, B, L, (int)gtcrn_num_frames(L), nullptr, d_win, tw, nullptr, 0, 0, 0, d_frames,
                                (hipStream_t)stream));
    return 0;
}

int gtcrn_istft(const float* d_spec, long sb, long sf, long st, int B, int T, const float* d_win, float* d_wave,
                void* stream) {
    if (!d_spec || !d_win || !d_wave || B < 1) return fail(GTCRN_ERR_ARG, "null pointer or B < 1");
    if (T < 2) return fail(GTCRN_ERR_ARG, "iSTFT needs T >= 2 frames");
    if (int rc0 = check_spec_layout(d_spec, sb, sf, st)) return rc0;
    float* tw = nullptr;
    int rc = device_twiddles(&tw);
    if (rc) return rc;
    LAUNCH_TRY(gtk::launch_istft(d_spec, sb, sf, st, B, T, nullptr, d_win, tw, d_wave, (hipStream_t)stream));
    return 0;
}

int gtcrn_forward_spec(gtcrn_model* m, const float* d_spec_in, long isb, long isf, long ist, float* d_spec_out,
                       long osb, long osf, long ost, int B, int T, void* stream) {
    int rc = check_model(m);
    if (rc) return rc;
    if (!d_spec_in || !d_spec_out) return fail(GTCRN_ERR_ARG, "null spectrogram pointer");
    if (B < 1 || T < 1) return fail(GTCRN_ERR_ARG, "B and T must be >= 1");
    if (int rc0 = check_spec_layout(d_spec_in, isb, isf, ist)) return rc0;
    if (int rc0 = check_spec_layout(d_spec_out, osb, osf, ost)) return rc0;
    hipStream_t s = (hipStream_t)stream;
    rc = ensure_workspace(m, B, T, s);
    if (rc) return rc;
    return run_model(m, d_spec_in, isb, isf, ist, d_spec_out, osb, osf, ost, B, T, nullptr, s);
}

// d_gain (optional): the attenuation limit, mixed by the iSTFT launch (k_istft_mix)
static int forward_wave_impl(gtcrn_model* m, const float* d_wave, float* d_wave_out, int B, long L,
                             const int* d_lengths, const float* d_win, void* stream,
                             const gtk::Quant* q = nullptr, const float* d_gain = nullptr) {
    int rc = check_model(m);
    if (rc) return rc;
    if (!d_wave || !d_wave_out || !d_win) return fail(GTCRN_ERR_ARG, "null pointer");
    if (B < 1) return fail(GTCRN_ERR_ARG, "B must be >= 1");
    if (L < 257) return fail(GTCRN_ERR_ARG, "reflect padding needs L > 256 samples");
    hipStream_t s = (hipStream_t)stream;
    const int T = (int)gtcrn_num_frames(L);
    rc = ensure_workspace(m, B, T, s);
    if (rc) return rc;
    // internal spectrograms are frame-major (B,T,257,2): sb = T*514, sf = 2, st = 514
    const long sb = (long)T * 514, sf = 2, st = 514;
    Timer tm(m, s);
    tm.begin(K_FRONT);
    LAUNCH_TRY(gtk::launch_front(d_wave, L, nullptr, 0, 0, 0, B, T, d_lengths, d_win, m->d_twid, q ? m->d_pfq : m->d_pf,
                                 m->d_pi, m->d_spec_a, m->d_en0, m->d_en[0], s, q));
    tm.end();
    rc = run_model(m, m->d_spec_a, sb, sf, st, m->d_spec_b, sb, sf, st, B, T, nullptr, s, d_lengths, q, true);
    if (rc) return rc;
    tm.begin(d_gain ? K_ISTFT_MIX : K_ISTFT);
    LAUNCH_TRY(gtk::launch_istft(m->d_spec_b, sb, sf, st, B, T, d_lengths, d_win, m->d_twid, d_wave_out, s, d_wave, L, d_gain));
    tm.end();
    return 0;
}

int gtcrn_forward_wave(gtcrn_model* m, const float* d_wave, float* d_wave_out, int B, long L, const float* d_win,
                       void* stream) {
    return forward_wave_impl(m, d_wave, d_wave_out, B, L, nullptr, d_win, stream);
}

int gtcrn_forward_wave_var(gtcrn_model* m, const float* d_wave, float* d_wave_out, int B, long Lmax,
                           const int* d_lengths, const float* d_win, void* stream) {
    if (!d_lengths) return fail(GTCRN_ERR_ARG, "gtcrn_forward_wave_var: null lengths");
    return forward_wave_impl(m, d_wave, d_wave_out, B, Lmax, d_lengths, d_win, stream);
}

int gtcrn_forward_wave_limited(gtcrn_model* m, const float* d_wave, float* d_wave_out, int B, long Lmax, const int* d_lengths,
                               const float* d_gain, const float* d_win, void* stream) {
    return forward_wave_impl(m, d_wave, d_wave_out, B, Lmax, d_lengths, d_win, stream, nullptr, d_gain);
}

static int quant_opts(float in_scale, float out_scale, gtk::Quant* q) {
    if (in_scale < 0.f || out_scale < 0.f) return fail(GTCRN_ERR_ARG, "quantiser scales must be >= 0 (0 = fp16 boundary)");
    q->in_step = in_scale / 255.0f;     // calibration maps [-scale/2, scale/2] onto the 255 int8 steps
    q->out_step = out_scale / 255.0f;
    return 0;
}

int gtcrn_forward_spec_quant(gtcrn_model* m, const float* d_spec_in, long isb, long isf, long ist, float* d_spec_out,
                             long osb, long osf, long ost, int B, int T, float in_scale, float out_scale, void* stream) {
    int rc = check_model(m);
    if (rc) return rc;
    if (!d_spec_in || !d_spec_out) return fail(GTCRN_ERR_ARG, "null spectrogram pointer");
    if (B < 1 || T < 1) return fail(GTCRN_ERR_ARG, "B and T must be >= 1");
    if (int rc0 = check_spec_layout(d_spec_in, isb, isf, ist)) return rc0;
    if (int rc0 = check_spec_layout(d_spec_out, osb, osf, ost)) return rc0;
    gtk::Quant q;
    if ((rc = quant_opts(in_scale, out_scale, &q))) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = ensure_workspace(m, B, T, s);
    if (rc) return rc;
    return run_model(m, d_spec_in, isb, isf, ist, d_spec_out, osb, osf, ost, B, T, nullptr, s, nullptr, &q);
}

int gtcrn_forward_wave_quant(gtcrn_model* m, const float* d_wave, float* d_wave_out, int B, long L, const float* d_win,
                             float in_scale, float out_scale, void* stream) {
    gtk::Quant q;
    if (int rc = quant_opts(in_scale, out_scale, &q)) return rc;
    return forward_wave_impl(m, d_wave, d_wave_out, B, L, nullptr, d_win, stream, &q);
}

size_t gtcrn_stream_state_bytes(void) { return sizeof(float) * gtk::ST_FLOATS; }

int gtcrn_stream_reset(gtcrn_model* m, void* d_state, int nstreams, void* stream) {
    int rc = check_model(m);
    if (rc) return rc;
    if (!d_state || nstreams < 1) return fail(GTCRN_ERR_ARG, "null state or nstreams < 1");
    HIP_TRY(hipMemsetAsync(d_state, 0, gtcrn_stream_state_bytes() * nstreams, (hipStream_t)stream));
    return 0;
}

int gtcrn_stream_step(gtcrn_model* m, void* d_state, const float* d_spec_t, long isb, long isf, long ist,
                      float* d_spec_out_t, long osb, long osf, long ost, int nstreams, int nframes, void* stream) {
    int rc = check_model(m);
    if (rc) return rc;
    if (!d_state || !d_spec_t || !d_spec_out_t) return fail(GTCRN_ERR_ARG, "null pointer");
    if (nstreams < 1 || nframes < 1) return fail(GTCRN_ERR_ARG, "nstreams and nframes must be >= 1");
    if (int rc0 = check_spec_layout(d_spec_t, isb, isf, ist)) return rc0;
    if (int rc0 = check_spec_layout(d_spec_out_t, osb, osf, ost)) return rc0;
    hipStream_t s = (hipStream_t)stream;
    rc = ensure_workspace(m, nstreams, nframes, s);
    if (rc) return rc;
    return run_model(m, d_spec_t, isb, isf, ist, d_spec_out_t, osb, osf, ost, nstreams, nframes, (float*)d_state, s);
}

// ---- hop-level waveform streaming: analysis -> the model step on the frame-major spectra -> synthesis, on one stream.
// The hand-offs use the frame-major spectrogram workspace of forward_wave (d_spec_a / d_spec_b), which the streaming
// forms of run_model never touch; ensure_workspace(N, nhops) sizes them.
size_t gtcrn_wave_stream_state_bytes(void) { return sizeof(float) * gtk::WS_FLOATS; }

int gtcrn_wave_stream_reset(gtcrn_model* m, void* d_state, void* d_wstate, int nstreams, void* stream) {
    if (!m) return fail(GTCRN_ERR_ARG, "gtcrn_wave_stream_reset: null model");
    if (!d_state || !d_wstate || nstreams < 1) return fail(GTCRN_ERR_ARG, "gtcrn_wave_stream_reset: null state or nstreams < 1");
    int rc = check_model(m);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(d_state, 0, gtcrn_stream_state_bytes() * nstreams, (hipStream_t)stream));
    HIP_TRY(hipMemsetAsync(d_wstate, 0, gtcrn_wave_stream_state_bytes() * nstreams, (hipStream_t)stream));
    return 0;
}

// Level meters (contract: include/gtcrn_micro_hip.h, "level meters"): the model keeps the address, wave_step hands it to the
// synthesis launch.  Nothing is launched or read here.
int gtcrn_wave_stream_set_meters(gtcrn_model* m, float* d_meters) {
    if (!m) return fail(GTCRN_ERR_ARG, "gtcrn_wave_stream_set_meters: null model");
    if (reinterpret_cast<uintptr_t>(d_meters) & 15)
        return fail(GTCRN_ERR_ARG, "gtcrn_wave_stream_set_meters: the records must be 16-byte aligned");
    m->live.meters = d_meters;
    return 0;
}

// Gain ramps (contract: include/gtcrn_micro_hip.h, "gain ramps"): kept like the meters' address; wave_step hands it to the
// synthesis launch of a call that has gains.  Nothing is launched or read here.
int gtcrn_wave_stream_set_gain_ramp(gtcrn_model* m, float* d_ramp) {
    if (!m) return fail(GTCRN_ERR_ARG, "gtcrn_wave_stream_set_gain_ramp: null model");
    m->live.ramp = d_ramp;
    return 0;
}
// the host twin: the 256 gains of a block that ramps from p to g, from the function the kernel compiles
int gtcrn_gain_ramp_host(float p, float g, float* out256) {
    if (!out256) return fail(GTCRN_ERR_ARG, "gtcrn_gain_ramp_host: null pointer");
    for (int i = 0; i < 256; ++i) out256[i] = gtk::gain_ramp_at(p, g, i);
    return 0;
}

// Level control (contract: include/gtcrn_micro_hip.h, "level control"): both addresses are kept like the meters'; wave_step
// hands them to the synthesis launch.  Nothing is launched or read here.
int gtcrn_wave_stream_set_alc(gtcrn_model* m, float* d_alc, const float* d_alc_params) {
    if (!m) return fail(GTCRN_ERR_ARG, "gtcrn_wave_stream_set_alc: null model");
    if (!d_alc != !d_alc_params) return fail(GTCRN_ERR_ARG, "gtcrn_wave_stream_set_alc: the records and the parameters come together");
    if (reinterpret_cast<uintptr_t>(d_alc) & 31)
        return fail(GTCRN_ERR_ARG, "gtcrn_wave_stream_set_alc: the records must be 32-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_alc_params) & 15)
        return fail(GTCRN_ERR_ARG, "gtcrn_wave_stream_set_alc: the parameters must be 16-byte aligned");
    m->live.alc = d_alc;
    m->live.alc_params = d_alc_params;
    return 0;
}
// the parameter words of a configuration: double arithmetic, one rounding to float each
int gtcrn_alc_params_host(const gtcrn_alc_config* c, float* out16) {
    if (!c || !out16) return fail(GTCRN_ERR_ARG, "gtcrn_alc_params_host: null pointer");
    const double v[] = {c->target_dbov, c->min_gain_db, c->max_gain_db, c->rise_db_s, c->fall_db_s, c->ceiling_dbov,
                        c->floor_dbov, c->ratio_db, c->hang_ms, c->alpha};
    for (double x : v)
        if (!std::isfinite(x)) return fail(GTCRN_ERR_ARG, "gtcrn_alc_params_host: a field is not finite");
    if (c->min_gain_db > c->max_gain_db) return fail(GTCRN_ERR_ARG, "gtcrn_alc_params_host: min_gain_db above max_gain_db");
    if (c->rise_db_s < 0 || c->fall_db_s < 0) return fail(GTCRN_ERR_ARG, "gtcrn_alc_params_host: a negative slew rate");
    if (c->hang_ms < 0 || c->hang_ms > 16.0 * (1 << 24)) return fail(GTCRN_ERR_ARG, "gtcrn_alc_params_host: hang_ms out of range");
    if (c->alpha < 0 || c->alpha > 1) return fail(GTCRN_ERR_ARG, "gtcrn_alc_params_host: alpha outside [0, 1]");
    if (c->mode != 0 && c->mode != 1) return fail(GTCRN_ERR_ARG, "gtcrn_alc_params_host: mode must be 0 or 1");
    const auto p10 = [](double db, double div) { return std::pow(10.0, db / div); };
    const auto fin = [](double x) { return (float)std::min(x, (double)FLT_MAX); };
    for (int i = 0; i < 16; ++i) out16[i] = 0.f;
    out16[0] = std::max(fin(256.0 * p10(c->floor_dbov, 10)), 1e-30f);
    out16[1] = fin(p10(c->ratio_db, 10));
    out16[2] = (float)std::ceil(c->hang_ms / 16.0);
    out16[3] = (float)c->alpha;
    out16[4] = fin(256.0 * p10(c->target_dbov, 10));
    out16[5] = std::min(std::max(fin(p10(c->min_gain_db, 20)), FLT_MIN), 1.0f);
    out16[6] = std::max(fin(p10(c->max_gain_db, 20)), 1.0f);
    out16[7] = fin(p10(c->rise_db_s * 0.016, 20));
    out16[8] = (float)p10(-c->fall_db_s * 0.016, 20);
    out16[9] = fin(p10(c->ceiling_dbov, 20));
    out16[10] = (float)c->mode;
    return 0;
}
// the host twin: one emitted block through the functions the kernel compiles (lane l holds samples 2l, 2l + 1, 128 + 2l,
// 129 + 2l; the reductions run the xor butterfly over lane distances 1 .. 32)
int gtcrn_alc_block_host(const float* params16, float* record8, const float* w256, const float* x256, const float* m256,
                         float* y256) {
    if (!params16 || !record8 || !w256 || !x256 || !m256 || !y256) return fail(GTCRN_ERR_ARG, "gtcrn_alc_block_host: null pointer");
    const auto butterfly = [](float* v, bool sum) {
        for (int d = 1; d < 64; d <<= 1) {
            float t[64];
            for (int l = 0; l < 64; ++l) t[l] = sum ? v[l] + v[l ^ d] : std::fmax(v[l], v[l ^ d]);
            for (int l = 0; l < 64; ++l) v[l] = t[l];
        }
        return v[0];
    };
    float ew[64], ex[64], pk[64];
    for (int l = 0; l < 64; ++l) {
        const int i[4] = {2 * l, 2 * l + 1, 128 + 2 * l, 129 + 2 * l};
        ew[l] = gtk::alc_lane_sum(w256[i[0]], w256[i[1]], w256[i[2]], w256[i[3]]);
        ex[l] = gtk::alc_lane_sum(x256[i[0]], x256[i[1]], x256[i[2]], x256[i[3]]);
        pk[l] = std::fmax(std::fmax(std::fabs(m256[i[0]]), std::fabs(m256[i[1]])),
                          std::fmax(std::fabs(m256[i[2]]), std::fabs(m256[i[3]])));
    }
    const float* p = params16;
    const gtk::AlcParams P{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10]};
    gtk::AlcRecord R{record8[0], record8[1], record8[2], record8[3], record8[4], record8[5]};
    float a0, a1;
    gtk::alc_decide(P, R, butterfly(ew, true), butterfly(ex, true), butterfly(pk, false), a0, a1);
    for (int i = 0; i < 256; ++i) {
        const float gi = gtk::gain_ramp_at(a0, a1, i);
        y256[i] = gi * m256[i];
    }
    const float rec[8] = {R.a, R.S, R.hang, R.voice, R.voiced, R.blocks, 0.f, 0.f};
    for (int i = 0; i < 8; ++i) record8[i] = rec[i];
    return 0;
}

// Tone guard (contract: include/gtcrn_micro_hip.h, "tone guard"): the three addresses are kept like the meters'; wave_step
// hands them to the synthesis launch.  Nothing is launched or read here.
int gtcrn_wave_stream_set_tone(gtcrn_model* m, float* d_tone, const float* d_tone_params, const float* d_tone_table) {
    if (!m) return fail(GTCRN_ERR_ARG, "gtcrn_wave_stream_set_tone: null model");
    if (!d_tone != !d_tone_params || !d_tone != !d_tone_table)
        return fail(GTCRN_ERR_ARG, "gtcrn_wave_stream_set_tone: the records, the parameters and the table come together");
    if (reinterpret_cast<uintptr_t>(d_tone) & 31)
        return fail(GTCRN_ERR_ARG, "gtcrn_wave_stream_set_tone: the records must be 32-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_tone_params) | reinterpret_cast<uintptr_t>(d_tone_table)) & 15)
        return fail(GTCRN_ERR_ARG, "gtcrn_wave_stream_set_tone: the parameters and the table must be 16-byte aligned");
    m->live.tone = d_tone;
    m->live.tone_params = d_tone_params;
    m->live.tone_table = d_tone_table;
    return 0;
}
// the table: cos and sin of 2 pi F_f i / 16000 in double, rounded once
int gtcrn_tone_table_host(float* out) {
    if (!out) return fail(GTCRN_ERR_ARG, "gtcrn_tone_table_host: null pointer");
    constexpr double F[gtk::TONE_FREQS] = {697, 770, 852, 941, 1209, 1336, 1477, 1633, 1100, 2100};
    const double two_pi = 6.283185307179586476925286766559;
    for (int f = 0; f < gtk::TONE_FREQS; ++f)
        for (int i = 0; i < 256; ++i) {
            const double a = two_pi * F[f] * i / 16000.0;
            out[(f * 256 + i) * 2] = (float)std::cos(a);
            out[(f * 256 + i) * 2 + 1] = (float)std::sin(a);
        }
    return 0;
}
// the parameter words of a configuration: double arithmetic, one rounding to float each
int gtcrn_tone_params_host(const gtcrn_tone_config* c, float* out16) {
    if (!c || !out16) return fail(GTCRN_ERR_ARG, "gtcrn_tone_params_host: null pointer");
    for (double x : {c->min_dbov, c->twist_db, c->dominance_db, c->pair_purity, c->single_purity})
        if (!std::isfinite(x)) return fail(GTCRN_ERR_ARG, "gtcrn_tone_params_host: a field is not finite");
    for (double x : {c->pair_purity, c->single_purity})
        if (!(x > 0 && x <= 1)) return fail(GTCRN_ERR_ARG, "gtcrn_tone_params_host: a purity outside (0, 1]");
    for (int k : {c->guard_blocks, c->digit_blocks, c->single_blocks, c->hold_blocks})
        if (k < 0 || k > (1 << 24)) return fail(GTCRN_ERR_ARG, "gtcrn_tone_params_host: a count is negative or above 2^24");
    if ((c->mode != 0 && c->mode != 1) || (c->singles != 0 && c->singles != 1))
        return fail(GTCRN_ERR_ARG, "gtcrn_tone_params_host: mode and singles must be 0 or 1");
    const auto fin = [](double x) { return (float)std::min(x, (double)FLT_MAX); };
    for (int i = 0; i < 16; ++i) out16[i] = 0.f;
    out16[0] = fin(256.0 * std::pow(10.0, c->min_dbov / 10));
    out16[1] = fin(std::pow(10.0, c->twist_db / 10));
    out16[2] = fin(std::pow(10.0, -c->dominance_db / 10));
    out16[3] = (float)c->pair_purity;
    out16[4] = (float)c->single_purity;
    out16[5] = (float)c->guard_blocks;
    out16[6] = (float)c->digit_blocks;
    out16[7] = (float)c->single_blocks;
    out16[8] = (float)c->hold_blocks;
    out16[9] = (float)c->mode;
    out16[10] = (float)c->singles;
    return 0;
}
// the host twin: steps 1 and 3 .. 5 of one emitted block through the functions the kernel compiles (lane l holds samples 2l,
// 2l + 1, 128 + 2l, 129 + 2l; the reductions run the xor butterfly over lane distances 1 .. 32)
int gtcrn_tone_block_host(const float* params16, const float* table, float* record8, const float* x256, int* guard_out) {
    if (!params16 || !table || !record8 || !x256 || !guard_out) return fail(GTCRN_ERR_ARG, "gtcrn_tone_block_host: null pointer");
    const auto butterfly = [](float* v) {
        for (int d = 1; d < 64; d <<= 1) {
            float t[64];
            for (int l = 0; l < 64; ++l) t[l] = v[l] + v[l ^ d];
            for (int l = 0; l < 64; ++l) v[l] = t[l];
        }
        return v[0];
    };
    float v[64], w[64], P[gtk::TONE_FREQS];
    for (int l = 0; l < 64; ++l) v[l] = gtk::alc_lane_sum(x256[2 * l], x256[2 * l + 1], x256[128 + 2 * l], x256[129 + 2 * l]);
    const float ex = butterfly(v);
    for (int f = 0; f < gtk::TONE_FREQS; ++f) {
        const float* t = table + 512 * f;
        for (int l = 0; l < 64; ++l) {
            const int i[4] = {2 * l, 2 * l + 1, 128 + 2 * l, 129 + 2 * l};
            v[l] = gtk::tone_lane_dot(x256[i[0]], x256[i[1]], x256[i[2]], x256[i[3]], t[2 * i[0]], t[2 * i[1]], t[2 * i[2]], t[2 * i[3]]);
            w[l] = gtk::tone_lane_dot(x256[i[0]], x256[i[1]], x256[i[2]], x256[i[3]], t[2 * i[0] + 1], t[2 * i[1] + 1],
                                      t[2 * i[2] + 1], t[2 * i[3] + 1]);
        }
        const float cf = butterfly(v), sf = butterfly(w);
        P[f] = gtk::tone_power(cf, sf);
    }
    const float* p = params16;
    const gtk::ToneParams TP{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10]};
    float* r = record8;
    gtk::ToneRecord R{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
    gtk::tone_decide(TP, R, ex, P);
    const float rec[8] = {R.tone, R.cand, R.run, R.hold, R.guard, R.events, R.guarded, R.blocks};
    for (int i = 0; i < 8; ++i) record8[i] = rec[i];
    *guard_out = TP.mode == 1.f && R.guard != 0.f;
    return 0;
}

// RFC 6464 audio level of a window of `nsamples` samples with energy `energy` (full scale 1.0): -dBov rounded to the nearest
// integer, 0 (loudest) .. 127 (silence).  Host arithmetic only.
int gtcrn_level_dbov(double energy, double nsamples) {
    if (!(energy > 0.0) || !(nsamples > 0.0)) return 127;
    const double l = std::floor(-10.0 * std::log10(energy / nsamples) + 0.5);
    return l < 0.0 ? 0 : l > 127.0 ? 127 : (int)l;
}

// Stream slots (contract: include/gtcrn_micro_hip.h): row i of a call is the stream whose states sit in slot d_slots[i];
// *d_count rows (clamped to 0..max_active on the device) step.  The host sizes the grid, the workspace and the form from
// max_active alone, so one captured graph serves any active set.  Only the single-launch step exists indexed.
namespace {
int slots_args(const std::string& w, gtcrn_model* m, const void* d_state, const void* d_wstate, const int* d_slots,
               int max_active) {
    if (!m) return fail(GTCRN_ERR_ARG, w + ": null model");
    if (!d_state || !d_slots) return fail(GTCRN_ERR_ARG, w + ": null pointer");
    if (max_active < 1) return fail(GTCRN_ERR_ARG, w + ": max_active must be >= 1");
    return check_state_alignment(w, {d_state, d_wstate});
}
int refuse_three_launch_form(const std::string& w, const gtcrn_model* m) {
    if (fused_stream_allowed(m)) return 0;
    return fail(GTCRN_ERR_STATE, w + ": the three-launch form (gtcrn_stream_form 1, gtcrn_debug_enable 1) has no indexed step");
}
}  // namespace

// Every gtcrn_wave_stream_* entry point: analysis -> the model step -> synthesis of n rows; the rate, packet and packet-slot
// forms come through here too.  The synthesis takes the model's buffers (m->live) and the call's d_gain as one gtk::WaveOpts;
// gtk::synth_mode picks the kernel from it and gtk::synth_timed_as the timing row.  Without a table the rows are the n
// streams of a contiguous state range, nhops hops each; with one (the _slots calls) the n = max_active rows it names, one hop.
extern "C++" template <typename S>
static int wave_step(const char* who, gtcrn_model* m, void* d_state, void* d_wstate, const S* d_in, long in_stride, S* d_out,
                     long out_stride, int n, int nhops, bool flush, int r, const float* d_gain, const float* d_win,
                     gtk::Rows rows, void* stream) {
    const std::string w(who);
    const bool indexed = rows.slots != nullptr;
    if (!m) return fail(GTCRN_ERR_ARG, w + ": null model");
    if (!d_state || !d_wstate || !d_out || !d_win || (!d_in && !(flush && r == 0)))
        return fail(GTCRN_ERR_ARG, w + ": null pointer");
    if (n < 1 || nhops < 1)
        return fail(GTCRN_ERR_ARG, w + (indexed ? ": max_active must be >= 1" : ": nstreams and nhops must be >= 1"));
    if (flush && (r < 0 || r > 255)) return fail(GTCRN_ERR_ARG, w + ": the tail holds r = 0..255 samples");
    if (in_stride < (flush ? r : 256L * nhops) || out_stride < 256L * (flush ? 1 : nhops))
        return fail(GTCRN_ERR_ARG, w + ": a stride is shorter than its row");
    if (int rc0 = check_state_alignment(w, {d_state, d_wstate})) return rc0;
    int rc = check_model(m);
    if (rc) return rc;
    if (indexed && (rc = refuse_three_launch_form(w, m))) return rc;      // (before the analysis launch: nothing runs on a refusal)
    hipStream_t s = (hipStream_t)stream;
    rc = ensure_workspace(m, n, nhops, s);
    if (rc) return rc;
    const long sb = (long)nhops * 514, sf = 2, st = 514;      // frame-major (n, nhops, 257, 2)
    float* ws = static_cast<float*>(d_wstate);
    float* ms = static_cast<float*>(d_state);
    Timer tm(m, s);
    tm.begin(K_WAVE_ANALYSIS);
    LAUNCH_TRY(gtk::launch_wave_analysis<S>(d_in, in_stride, n, nhops, r, flush, ws, d_win, m->d_twid, m->d_spec_a, rows, s));
    tm.end();
    rc = indexed ? fused_stream_step(m, m->d_spec_a, sb, sf, m->d_spec_b, sb, sf, n, ms, rows, s)
                 : run_model(m, m->d_spec_a, sb, sf, st, m->d_spec_b, sb, sf, st, n, nhops, ms, s);
    if (rc) return rc;
    gtk::WaveOpts o = m->live;
    o.gain = d_gain;
    constexpr int row[] = {K_WAVE_SYNTHESIS, K_WAVE_SYNTHESIS_MIX, K_WAVE_SYNTHESIS_METER};      // Synth::Plain, Mix, Meter
    tm.begin(row[(int)gtk::synth_timed_as(o)]);
    LAUNCH_TRY(gtk::launch_wave_synthesis<S>(m->d_spec_b, d_in, in_stride, d_out, out_stride, n, nhops, r, flush, ws, d_win,
                                             m->d_twid, rows, o, s));
    tm.end();
    return 0;
}
// a _slots entry point: one hop of the max_active rows the table names
extern "C++" template <typename S>
static int wave_step_slots(const char* who, gtcrn_model* m, void* d_state, void* d_wstate, const int* d_slots,
                           const int* d_count, int max_active, const S* d_in, long in_stride, S* d_out, long out_stride,
                           bool flush, int r, const float* d_gain, const float* d_win, void* stream) {
    if (m && !d_slots) return fail(GTCRN_ERR_ARG, std::string(who) + ": null pointer");
    return wave_step<S>(who, m, d_state, d_wstate, d_in, in_stride, d_out, out_stride, max_active, 1, flush, r, d_gain, d_win,
                        gtk::Rows{d_slots, d_count}, stream);
}

int gtcrn_wave_stream_step(gtcrn_model* m, void* d_state, void* d_wstate, const float* d_in, long in_stride, float* d_out,
                           long out_stride, int nstreams, int nhops, const float* d_win, void* stream) {
    return wave_step<float>("gtcrn_wave_stream_step", m, d_state, d_wstate, d_in, in_stride, d_out, out_stride,
                            nstreams, nhops, false, 0, nullptr, d_win, {}, stream);
}
int gtcrn_wave_stream_step_pcm16(gtcrn_model* m, void* d_state, void* d_wstate, const short* d_in, long in_stride,
                                 short* d_out, long out_stride, int nstreams, int nhops, const float* d_win, void* stream) {
    return wave_step<short>("gtcrn_wave_stream_step_pcm16", m, d_state, d_wstate, d_in, in_stride, d_out, out_stride,
                            nstreams, nhops, false, 0, nullptr, d_win, {}, stream);
}
int gtcrn_wave_stream_flush(gtcrn_model* m, void* d_state, void* d_wstate, const float* d_tail, long tail_stride, int r,
                            float* d_out, long out_stride, int nstreams, const float* d_win, void* stream) {
    return wave_step<float>("gtcrn_wave_stream_flush", m, d_state, d_wstate, d_tail, tail_stride, d_out, out_stride,
                            nstreams, 1, true, r, nullptr, d_win, {}, stream);
}
int gtcrn_wave_stream_flush_pcm16(gtcrn_model* m, void* d_state, void* d_wstate, const short* d_tail, long tail_stride, int r,
                                  short* d_out, long out_stride, int nstreams, const float* d_win, void* stream) {
    return wave_step<short>("gtcrn_wave_stream_flush_pcm16", m, d_state, d_wstate, d_tail, tail_stride, d_out,
                            out_stride, nstreams, 1, true, r, nullptr, d_win, {}, stream);
}

// the attenuation-limited forms: d_gain holds one dry gain per stream (NULL: the plain call)
int gtcrn_wave_stream_step_limited(gtcrn_model* m, void* d_state, void* d_wstate, const float* d_in, long in_stride,
                                   float* d_out, long out_stride, int nstreams, int nhops, const float* d_gain,
                                   const float* d_win, void* stream) {
    return wave_step<float>("gtcrn_wave_stream_step_limited", m, d_state, d_wstate, d_in, in_stride, d_out, out_stride,
                            nstreams, nhops, false, 0, d_gain, d_win, {}, stream);
}
int gtcrn_wave_stream_step_limited_pcm16(gtcrn_model* m, void* d_state, void* d_wstate, const short* d_in, long in_stride,
                                         short* d_out, long out_stride, int nstreams, int nhops, const float* d_gain,
                                         const float* d_win, void* stream) {
    return wave_step<short>("gtcrn_wave_stream_step_limited_pcm16", m, d_state, d_wstate, d_in, in_stride, d_out,
                            out_stride, nstreams, nhops, false, 0, d_gain, d_win, {}, stream);
}
int gtcrn_wave_stream_flush_limited(gtcrn_model* m, void* d_state, void* d_wstate, const float* d_tail, long tail_stride,
                                    int r, float* d_out, long out_stride, int nstreams, const float* d_gain,
                                    const float* d_win, void* stream) {
    return wave_step<float>("gtcrn_wave_stream_flush_limited", m, d_state, d_wstate, d_tail, tail_stride, d_out,
                            out_stride, nstreams, 1, true, r, d_gain, d_win, {}, stream);
}
int gtcrn_wave_stream_flush_limited_pcm16(gtcrn_model* m, void* d_state, void* d_wstate, const short* d_tail, long tail_stride,
                                          int r, short* d_out, long out_stride, int nstreams, const float* d_gain,
                                          const float* d_win, void* stream) {
    return wave_step<short>("gtcrn_wave_stream_flush_limited_pcm16", m, d_state, d_wstate, d_tail, tail_stride, d_out,
                            out_stride, nstreams, 1, true, r, d_gain, d_win, {}, stream);
}

// ---- stream slots: the same steps for the rows a call names (slots_args, wave_step_slots above) ---------------------------
int gtcrn_stream_step_slots(gtcrn_model* m, void* d_state, const int* d_slots, const int* d_count, int max_active,
                            const float* d_spec_t, long isb, long isf, long ist, float* d_spec_out_t, long osb, long osf,
                            long ost, void* stream) {
    const std::string w("gtcrn_stream_step_slots");
    if (int rc0 = slots_args(w, m, d_state, nullptr, d_slots, max_active)) return rc0;
    if (!d_spec_t || !d_spec_out_t) return fail(GTCRN_ERR_ARG, w + ": null pointer");
    if (int rc0 = check_spec_layout(d_spec_t, isb, isf, ist)) return rc0;
    if (int rc0 = check_spec_layout(d_spec_out_t, osb, osf, ost)) return rc0;
    int rc = check_model(m);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = ensure_workspace(m, max_active, 1, s);
    if (rc) return rc;
    if ((rc = refuse_three_launch_form(w, m))) return rc;
    if (!gtk::stream_ms_usable(isb, osb)) return fail(GTCRN_ERR_ARG, w + ": spectrogram row strides too large");
    return fused_stream_step(m, d_spec_t, isb, isf, d_spec_out_t, osb, osf, max_active, static_cast<float*>(d_state),
                             gtk::Rows{d_slots, d_count}, s);
}

int gtcrn_stream_reset_slots(gtcrn_model* m, void* d_state, void* d_wstate, const int* d_slots, const int* d_count,
                             int max_active, void* stream) {
    const std::string w("gtcrn_stream_reset_slots");
    if (int rc0 = slots_args(w, m, d_state, d_wstate, d_slots, max_active)) return rc0;
    int rc = check_model(m);
    if (rc) return rc;
    LAUNCH_TRY(gtk::launch_reset_slots(static_cast<float*>(d_state), static_cast<float*>(d_wstate), d_slots, d_count, max_active,
                                       (hipStream_t)stream));
    return 0;
}

int gtcrn_wave_stream_step_slots(gtcrn_model* m, void* d_state, void* d_wstate, const int* d_slots, const int* d_count,
                                 int max_active, const float* d_in, long in_stride, float* d_out, long out_stride,
                                 const float* d_gain, const float* d_win, void* stream) {
    return wave_step_slots<float>("gtcrn_wave_stream_step_slots", m, d_state, d_wstate, d_slots, d_count, max_active, d_in,
                                  in_stride, d_out, out_stride, false, 0, d_gain, d_win, stream);
}
int gtcrn_wave_stream_step_slots_pcm16(gtcrn_model* m, void* d_state, void* d_wstate, const int* d_slots, const int* d_count,
                                       int max_active, const short* d_in, long in_stride, short* d_out, long out_stride,
                                       const float* d_gain, const float* d_win, void* stream) {
    return wave_step_slots<short>("gtcrn_wave_stream_step_slots_pcm16", m, d_state, d_wstate, d_slots, d_count, max_active,
                                  d_in, in_stride, d_out, out_stride, false, 0, d_gain, d_win, stream);
}
int gtcrn_wave_stream_flush_slots(gtcrn_model* m, void* d_state, void* d_wstate, const int* d_slots, const int* d_count,
                                  int max_active, const float* d_tail, long tail_stride, int r, float* d_out, long out_stride,
                                  const float* d_gain, const float* d_win, void* stream) {
    return wave_step_slots<float>("gtcrn_wave_stream_flush_slots", m, d_state, d_wstate, d_slots, d_count, max_active, d_tail,
                                  tail_stride, d_out, out_stride, true, r, d_gain, d_win, stream);
}
int gtcrn_wave_stream_flush_slots_pcm16(gtcrn_model* m, void* d_state, void* d_wstate, const int* d_slots, const int* d_count,
                                        int max_active, const short* d_tail, long tail_stride, int r, short* d_out,
                                        long out_stride, const float* d_gain, const float* d_win, void* stream) {
    return wave_step_slots<short>("gtcrn_wave_stream_flush_slots_pcm16", m, d_state, d_wstate, d_slots, d_count, max_active,
                                  d_tail, tail_stride, d_out, out_stride, true, r, d_gain, d_win, stream);
}

// ---- sample-rate conversion ------------------------------------------------------------------------------------------
// The filter of include/gtcrn_micro_hip.h, designed here in double and rounded once to float: the kernels, the tests and
// gtcrn_resample_taps all see these coefficients.
namespace {

struct RsDesign {
    int up = 1, down = 1, half = 0;
    int nt = 1, ntp = 4;            // taps of the longest phase; the same rounded up to a multiple of 4 (the table's row)
    std::vector<float> h;           // 2 half + 1 taps
};

bool rs_rate_ok(int fs) {
    for (int r : {8000, 11025, 22050, 24000, 32000, 44100, 48000})
        if (fs == r) return true;
    return false;
}
bool rs_pair_ok(int fs_in, int fs_out) {
    return (fs_in == 16000 && (fs_out == 16000 || rs_rate_ok(fs_out))) || (fs_out == 16000 && rs_rate_ok(fs_in));
}
double bessel_i0(double x) {        // sum over k of ((x / 2)^k / k!)^2: every term positive, converges for all x
    const double y = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= y / ((double)k * (double)k);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}
void rs_ratio(int fs_in, int fs_out, int* up, int* down) {
    int a = fs_out, b = fs_in;
    while (b) { const int t = a % b; a = b; b = t; }
    *up = fs_out / a;
    *down = fs_in / a;
}
void rs_design(int fs_in, int fs_out, RsDesign* d, bool taps) {
    rs_ratio(fs_in, fs_out, &d->up, &d->down);
    if (fs_in == fs_out) {          // the no-op: one tap of 1
        d->half = 0; d->nt = 1; d->ntp = 4;
        if (taps) d->h.assign(1, 1.0f);
        return;
    }
    const int q = d->up > d->down ? d->up : d->down;
    d->half = 32 * q;
    d->nt = 2 * d->half / d->up + 1;
    d->ntp = (d->nt + 3) & ~3;
    if (!taps) return;
    const int n = 2 * d->half + 1;
    const double kPi = 3.14159265358979323846, beta = 8.95926, fc = 0.9375 * 0.5 / q, i0b = bessel_i0(beta);
    std::vector<double> h(n);
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
        const int k = i - d->half;
        const double x = 2.0 * fc * k, y = kPi * x, r = (double)k / (double)d->half;
        const double w = bessel_i0(beta * std::sqrt(1.0 - r * r)) / i0b;
        h[i] = (k == 0 ? 1.0 : std::sin(y) / y) * w;
        sum += h[i];
    }
    d->h.resize(n);
    for (int i = 0; i < n; ++i) d->h[i] = (float)(h[i] * ((double)d->up / sum));
}
// live rates: a hop of 256 samples at 16 kHz and the 32-period stage delay are whole numbers of samples at fs
bool rs_live_ok(int fs) { return fs == 8000 || fs == 24000 || fs == 32000 || fs == 48000; }

}  // namespace

struct gtcrn_resampler {
    int device = 0, fs_in = 0, fs_out = 0;
    RsDesign d;                     // (taps dropped after the upload)
    float* d_taps = nullptr;        // phase table: up rows of ntp floats, row k0 = h[k0], h[k0 + up], ... then +0.0f
};

long gtcrn_resample_taps(int fs_in, int fs_out, int* up, int* down, float* h_taps, long cap) {
    if (!rs_pair_ok(fs_in, fs_out))
        return fail(GTCRN_ERR_ARG, "gtcrn_resample_taps: supported rates are 8000, 11025, 22050, 24000, 32000, 44100, 48000 to / from 16000");
    RsDesign d;
    rs_design(fs_in, fs_out, &d, h_taps != nullptr);
    if (up) *up = d.up;
    if (down) *down = d.down;
    const long n = 2L * d.half + 1;
    if (h_taps) {
        if (cap < n) return fail(GTCRN_ERR_ARG, "gtcrn_resample_taps: the buffer holds fewer than 2 half + 1 taps");
        std::memcpy(h_taps, d.h.data(), sizeof(float) * n);
    }
    return n;
}

// Library-internal, like gtcrn_set_error_ (not in the header, no contract): the same design for any ratio.  metrics_host.cpp
// takes the scorer's 16 kHz -> 10 kHz stage from it, which is no rate of gtcrn_resample.
extern "C" long gtcrn_resample_design_(int fs_in, int fs_out, int* up, int* down, float* h_taps, long cap) {
    if (fs_in < 1 || fs_out < 1) return fail(GTCRN_ERR_ARG, "gtcrn_resample_design_: rates must be positive");
    RsDesign d;
    rs_design(fs_in, fs_out, &d, h_taps != nullptr);
    if (up) *up = d.up;
    if (down) *down = d.down;
    const long n = 2L * d.half + 1;
    if (h_taps) {
        if (cap < n) return fail(GTCRN_ERR_ARG, "gtcrn_resample_design_: the buffer holds fewer than 2 half + 1 taps");
        std::memcpy(h_taps, d.h.data(), sizeof(float) * n);
    }
    return n;
}

long gtcrn_resample_out_len(int fs_in, int fs_out, long L) {
    if (!rs_pair_ok(fs_in, fs_out) || L < 0) return fail(GTCRN_ERR_ARG, "gtcrn_resample_out_len: unsupported rate pair or L < 0");
    int up, down;
    rs_ratio(fs_in, fs_out, &up, &down);
    return (L * up + down - 1) / down;
}

int gtcrn_resampler_create(gtcrn_resampler** out, int fs_in, int fs_out, int device) {
    if (!out) return fail(GTCRN_ERR_ARG, "gtcrn_resampler_create: null out pointer");
    *out = nullptr;
    if (!rs_pair_ok(fs_in, fs_out))
        return fail(GTCRN_ERR_ARG, "gtcrn_resampler_create: supported rates are 8000, 11025, 22050, 24000, 32000, 44100, 48000 to / from 16000");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(GTCRN_ERR_DEVICE, "no HIP device");
    if (device < 0 || device >= ndev) return fail(GTCRN_ERR_ARG, "gtcrn_resampler_create: no such device");
    gtcrn_resampler* r = new gtcrn_resampler;
    r->device = device; r->fs_in = fs_in; r->fs_out = fs_out;
    rs_design(fs_in, fs_out, &r->d, true);
    const RsDesign& d = r->d;
    if (gtk::resample_tile_span(d.up, d.down, d.ntp) > gtk::RS_SPAN) {
        delete r;
        return fail(GTCRN_ERR_ARG, "gtcrn_resampler_create: the ratio's input span exceeds the kernel's tile");
    }
    std::vector<float> P((size_t)d.up * d.ntp, 0.0f);
    for (int k0 = 0; k0 < d.up; ++k0)
        for (int t = 0; k0 + (long)t * d.up <= 2L * d.half; ++t) P[(size_t)k0 * d.ntp + t] = d.h[k0 + (size_t)t * d.up];
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(&r->d_taps, sizeof(float) * P.size());
    if (e == hipSuccess) e = hipMemcpy(r->d_taps, P.data(), sizeof(float) * P.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (r->d_taps) (void)hipFree(r->d_taps);
        delete r;
        return hip_fail(e, "gtcrn_resampler_create");
    }
    r->d.h.clear();
    *out = r;
    return 0;
}

void gtcrn_resampler_destroy(gtcrn_resampler* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    (void)hipDeviceSynchronize();
    if (r->d_taps) (void)hipFree(r->d_taps);
    delete r;
}

extern "C++" template <typename SI, typename SO>
static int resample_impl(const char* who, gtcrn_resampler* r, const SI* d_in, long in_stride, const int* d_lengths, long L,
                         SO* d_out, long out_stride, int B, void* stream) {
    const std::string w(who);
    if (!r || !r->d_taps) return fail(GTCRN_ERR_ARG, w + ": null resampler");
    if (!d_in || !d_out) return fail(GTCRN_ERR_ARG, w + ": null pointer");
    if (B < 1 || L < 1) return fail(GTCRN_ERR_ARG, w + ": B and L must be >= 1");
    const RsDesign& d = r->d;
    const long nout = (L * d.up + d.down - 1) / d.down;
    if (in_stride < L || out_stride < nout) return fail(GTCRN_ERR_ARG, w + ": a stride is shorter than its row");
    HIP_TRY(hipSetDevice(r->device));
    LAUNCH_TRY((gtk::launch_resample<SI, SO>(d_in, in_stride, d_lengths, L, d_out, out_stride, B, d.up, d.down, d.half, d.ntp,
                                             r->d_taps, static_cast<hipStream_t>(stream))));
    return 0;
}
int gtcrn_resample(gtcrn_resampler* r, const float* d_in, long in_stride, const int* d_lengths, long L, float* d_out,
                   long out_stride, int B, void* stream) {
    return resample_impl<float, float>("gtcrn_resample", r, d_in, in_stride, d_lengths, L, d_out, out_stride, B, stream);
}
int gtcrn_resample_pcm16_in(gtcrn_resampler* r, const short* d_in, long in_stride, const int* d_lengths, long L, float* d_out,
                            long out_stride, int B, void* stream) {
    return resample_impl<short, float>("gtcrn_resample_pcm16_in", r, d_in, in_stride, d_lengths, L, d_out, out_stride, B, stream);
}
int gtcrn_resample_pcm16_out(gtcrn_resampler* r, const float* d_in, long in_stride, const int* d_lengths, long L, short* d_out,
                             long out_stride, int B, void* stream) {
    return resample_impl<float, short>("gtcrn_resample_pcm16_out", r, d_in, in_stride, d_lengths, L, d_out, out_stride, B, stream);
}

// ---- hop-level streaming at the caller's rate: k_rate_in -> the three launches of the wave step -> k_rate_out
int gtcrn_rate_stream_hop(int fs) {
    if (!rs_live_ok(fs)) return fail(GTCRN_ERR_ARG, "gtcrn_rate_stream_hop: live rates are 8000, 24000, 32000, 48000");
    return (int)(256L * fs / 16000);
}
int gtcrn_rate_stream_latency(int fs) {
    if (!rs_live_ok(fs)) return fail(GTCRN_ERR_ARG, "gtcrn_rate_stream_latency: live rates are 8000, 24000, 32000, 48000");
    RsDesign d;
    rs_design(fs, 16000, &d, false);
    return (int)(256L * fs / 16000) + 2 * (d.half / d.up);
}
size_t gtcrn_rate_stream_state_bytes(int fs) {
    if (!rs_live_ok(fs)) { (void)fail(GTCRN_ERR_ARG, "gtcrn_rate_stream_state_bytes: live rates are 8000, 24000, 32000, 48000"); return 0; }
    RsDesign a, b;
    rs_design(fs, 16000, &a, false);
    rs_design(16000, fs, &b, false);
    return sizeof(float) * (size_t)(a.ntp + b.ntp);
}

namespace {
// high band: the rates above 16 kHz that have a hop form
bool hb_rate_ok(int fs) { return fs == 24000 || fs == 32000 || fs == 48000; }
// do any of the N input rows (len samples each, in_stride apart) share a byte with any of the N output rows?
extern "C++" template <typename S>
bool rows_overlap(const S* in, long in_stride, const S* out, long out_stride, long len, int N) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out);
    const uintptr_t ea = a + sizeof(S) * (uintptr_t)((long)(N - 1) * in_stride + len);
    const uintptr_t eb = b + sizeof(S) * (uintptr_t)((long)(N - 1) * out_stride + len);
    if (ea <= b || eb <= a) return false;                 // the two extents are disjoint
    if (in_stride != out_stride || (a > b ? a - b : b - a) % sizeof(S)) return true;      // (interleavings not analysed)
    const long d = (long)((a > b ? a - b : b - a) / sizeof(S)) % in_stride;              // rows interleaved at one pitch
    return d < len || in_stride - d < len;
}
int rate_pair_check(const std::string& w, gtcrn_model* m, gtcrn_resampler* in, gtcrn_resampler* out) {
    if (!m) return fail(GTCRN_ERR_ARG, w + ": null model");
    if (!in || !out || !in->d_taps || !out->d_taps) return fail(GTCRN_ERR_ARG, w + ": null resampler");
    if (in->fs_out != 16000 || out->fs_in != 16000 || in->fs_in != out->fs_out || !rs_live_ok(in->fs_in))
        return fail(GTCRN_ERR_ARG, w + ": the resamplers must be fs -> 16000 and 16000 -> fs, fs in {8000, 24000, 32000, 48000}");
    if (in->device != m->device || out->device != m->device) return fail(GTCRN_ERR_ARG, w + ": resamplers and model on different devices");
    return 0;
}
int ensure_rate_workspace(gtcrn_model* m, int nstreams, int nhops, hipStream_t s) {
    const long need = (long)nstreams * nhops;
    if (need <= m->cap_rate) return 0;
    if (int rc = before_growing(s, "rate hand-off buffers too small during stream capture: call gtcrn_rate_stream_reserve first"))
        return rc;
    if (m->d_rate_a) (void)hipFree(m->d_rate_a);
    if (m->d_rate_b) (void)hipFree(m->d_rate_b);
    m->d_rate_a = m->d_rate_b = nullptr;
    m->cap_rate = 0;
    HIP_TRY(hipMalloc(&m->d_rate_a, sizeof(float) * 256 * need));
    HIP_TRY(hipMalloc(&m->d_rate_b, sizeof(float) * 256 * need));
    m->cap_rate = need;
    return 0;
}
}  // namespace

int gtcrn_rate_stream_reserve(gtcrn_model* m, gtcrn_resampler* in, gtcrn_resampler* out, int nstreams, int nhops) {
    if (int rc = rate_pair_check("gtcrn_rate_stream_reserve", m, in, out)) return rc;
    if (nstreams < 1 || nhops < 1) return fail(GTCRN_ERR_ARG, "gtcrn_rate_stream_reserve: nstreams and nhops must be >= 1");
    int rc = check_model(m);
    if (rc) return rc;
    if ((rc = ensure_workspace(m, nstreams, nhops, nullptr))) return rc;
    return ensure_rate_workspace(m, nstreams, nhops, nullptr);
}

long gtcrn_rate_stream_debug_handoff(gtcrn_model* m, int which, float* d_dst, long n, void* stream) {
    if (!m || !d_dst || (which != 0 && which != 1) || n < 1)
        return fail(GTCRN_ERR_ARG, "gtcrn_rate_stream_debug_handoff: null pointer, n < 1 or which not 0 / 1");
    if (n > 256 * m->cap_rate) return fail(GTCRN_ERR_STATE, "gtcrn_rate_stream_debug_handoff: no rate step of that size has run");
    int rc = check_model(m);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d_dst, which ? m->d_rate_b : m->d_rate_a, sizeof(float) * n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return n;
}

int gtcrn_rate_stream_reset(gtcrn_model* m, gtcrn_resampler* in, gtcrn_resampler* out, void* d_state, void* d_wstate,
                            void* d_rstate, int nstreams, void* stream) {
    if (int rc = rate_pair_check("gtcrn_rate_stream_reset", m, in, out)) return rc;
    if (!d_rstate) return fail(GTCRN_ERR_ARG, "gtcrn_rate_stream_reset: null state or nstreams < 1");
    if (int rc = gtcrn_wave_stream_reset(m, d_state, d_wstate, nstreams, stream)) return rc;
    HIP_TRY(hipMemsetAsync(d_rstate, 0, gtcrn_rate_stream_state_bytes(in->fs_in) * nstreams, (hipStream_t)stream));
    return 0;
}

extern "C++" template <typename S>
static int rate_stream_impl(const char* who, gtcrn_model* m, gtcrn_resampler* in, gtcrn_resampler* out, void* d_state,
                            void* d_wstate, void* d_rstate, const S* d_in, long in_stride, S* d_out, long out_stride,
                            int nstreams, int nhops, const float* d_win, void* stream, const float* d_gain = nullptr,
                            bool hb = false, void* d_hbstate = nullptr, const float* d_hb_gain = nullptr) {
    const std::string w(who);
    if (int rc = rate_pair_check(w, m, in, out)) return rc;
    if (hb && !hb_rate_ok(in->fs_in)) return fail(GTCRN_ERR_ARG, w + ": the high band exists at 24000, 32000 and 48000 Hz");
    if (!d_state || !d_wstate || !d_rstate || !d_in || !d_out || !d_win) return fail(GTCRN_ERR_ARG, w + ": null pointer");
    if (hb && (!d_hbstate || !d_hb_gain)) return fail(GTCRN_ERR_ARG, w + ": null high-band state or gain pointer");
    if (nstreams < 1 || nhops < 1) return fail(GTCRN_ERR_ARG, w + ": nstreams and nhops must be >= 1");
    const int H = (int)(256L * in->fs_in / 16000);
    if (in_stride < (long)H * nhops || out_stride < (long)H * nhops) return fail(GTCRN_ERR_ARG, w + ": a stride is shorter than its row");
    if (int rc0 = check_state_alignment(w, {d_state, d_wstate, d_rstate, d_hbstate})) return rc0;
    // the high-band kernel reads x[n - latency] while other threads write out: no in-place call
    if (hb && rows_overlap(d_in, in_stride, d_out, out_stride, (long)H * nhops, nstreams))
        return fail(GTCRN_ERR_ARG, w + ": the input and output rows overlap (the high-band step is not legal in place)");
    int rc = check_model(m);
    if (rc) return rc;
    if (hb && m->live.alc)     // (the high band's formulas assume the 16 kHz hand-off at unit gain)
        return fail(GTCRN_ERR_STATE, w + ": the high band does not go together with level control (gtcrn_wave_stream_set_alc)");
    hipStream_t s = (hipStream_t)stream;
    if ((rc = ensure_workspace(m, nstreams, nhops, s))) return rc;
    if ((rc = ensure_rate_workspace(m, nstreams, nhops, s))) return rc;
    const RsDesign &di = in->d, &dout = out->d;
    float* rs = static_cast<float*>(d_rstate);
    const long rs_stride = di.ntp + dout.ntp, row = 256L * nhops;
    LAUNCH_TRY(gtk::launch_rate_in<S>(d_in, in_stride, m->d_rate_a, row, rs, rs_stride, nstreams, nhops, H, di.up, di.down,
                                      di.ntp, in->d_taps, s));
    rc = wave_step<float>("gtcrn_wave_stream_step", m, d_state, d_wstate, m->d_rate_a, row, m->d_rate_b, row, nstreams,
                          nhops, false, 0, d_gain, d_win, {}, stream);      // (the limit is mixed at 16 kHz)
    if (rc) return rc;
    if (hb) {
        LAUNCH_TRY(gtk::launch_rate_out_hb<S>(m->d_rate_b, m->d_rate_a, row, d_in, in_stride, d_out, out_stride, rs + di.ntp,
                                              rs_stride, static_cast<float*>(d_hbstate), d_hb_gain, nstreams, nhops, H,
                                              H + 2 * (di.half / di.up), dout.up, dout.down, dout.ntp, out->d_taps, s));
        return 0;
    }
    LAUNCH_TRY(gtk::launch_rate_out<S>(m->d_rate_b, row, d_out, out_stride, rs + di.ntp, rs_stride, nstreams, nhops, H, dout.up,
                                       dout.down, dout.ntp, out->d_taps, s));
    return 0;
}
int gtcrn_rate_stream_step(gtcrn_model* m, gtcrn_resampler* in, gtcrn_resampler* out, void* d_state, void* d_wstate,
                           void* d_rstate, const float* d_in, long in_stride, float* d_out, long out_stride, int nstreams,
                           int nhops, const float* d_win, void* stream) {
    return rate_stream_impl<float>("gtcrn_rate_stream_step", m, in, out, d_state, d_wstate, d_rstate, d_in, in_stride, d_out,
                                   out_stride, nstreams, nhops, d_win, stream);
}
int gtcrn_rate_stream_step_pcm16(gtcrn_model* m, gtcrn_resampler* in, gtcrn_resampler* out, void* d_state, void* d_wstate,
                                 void* d_rstate, const short* d_in, long in_stride, short* d_out, long out_stride,
                                 int nstreams, int nhops, const float* d_win, void* stream) {
    return rate_stream_impl<short>("gtcrn_rate_stream_step_pcm16", m, in, out, d_state, d_wstate, d_rstate, d_in, in_stride,
                                   d_out, out_stride, nstreams, nhops, d_win, stream);
}

int gtcrn_rate_stream_step_limited(gtcrn_model* m, gtcrn_resampler* in, gtcrn_resampler* out, void* d_state, void* d_wstate,
                                   void* d_rstate, const float* d_in, long in_stride, float* d_out, long out_stride,
                                   int nstreams, int nhops, const float* d_gain, const float* d_win, void* stream) {
    return rate_stream_impl<float>("gtcrn_rate_stream_step_limited", m, in, out, d_state, d_wstate, d_rstate, d_in, in_stride,
                                   d_out, out_stride, nstreams, nhops, d_win, stream, d_gain);
}
int gtcrn_rate_stream_step_limited_pcm16(gtcrn_model* m, gtcrn_resampler* in, gtcrn_resampler* out, void* d_state,
                                         void* d_wstate, void* d_rstate, const short* d_in, long in_stride, short* d_out,
                                         long out_stride, int nstreams, int nhops, const float* d_gain, const float* d_win,
                                         void* stream) {
    return rate_stream_impl<short>("gtcrn_rate_stream_step_limited_pcm16", m, in, out, d_state, d_wstate, d_rstate, d_in,
                                   in_stride, d_out, out_stride, nstreams, nhops, d_win, stream, d_gain);
}

// ---- high band: the rate step with k_rate_out_hb as its fifth launch; the batch kernel for the offline composition
size_t gtcrn_rate_stream_hb_state_bytes(int fs) {
    if (!hb_rate_ok(fs)) { (void)fail(GTCRN_ERR_ARG, "gtcrn_rate_stream_hb_state_bytes: the high band exists at 24000, 32000 and 48000 Hz"); return 0; }
    return sizeof(float) * (size_t)(256 + gtcrn_rate_stream_latency(fs));
}
int gtcrn_rate_stream_hb_reset(int fs, void* d_hbstate, int nstreams, void* stream) {
    if (!hb_rate_ok(fs)) return fail(GTCRN_ERR_ARG, "gtcrn_rate_stream_hb_reset: the high band exists at 24000, 32000 and 48000 Hz");
    if (!d_hbstate || nstreams < 1) return fail(GTCRN_ERR_ARG, "gtcrn_rate_stream_hb_reset: null state or nstreams < 1");
    if (int rc = check_state_alignment("gtcrn_rate_stream_hb_reset", {d_hbstate})) return rc;
    HIP_TRY(hipMemsetAsync(d_hbstate, 0, gtcrn_rate_stream_hb_state_bytes(fs) * nstreams, (hipStream_t)stream));
    return 0;
}
int gtcrn_rate_stream_step_hb(gtcrn_model* m, gtcrn_resampler* in, gtcrn_resampler* out, void* d_state, void* d_wstate,
                              void* d_rstate, const float* d_in, long in_stride, float* d_out, long out_stride, int nstreams,
                              int nhops, const float* d_gain, const float* d_win, void* d_hbstate, const float* d_hb_gain,
                              void* stream) {
    return rate_stream_impl<float>("gtcrn_rate_stream_step_hb", m, in, out, d_state, d_wstate, d_rstate, d_in, in_stride, d_out,
                                   out_stride, nstreams, nhops, d_win, stream, d_gain, true, d_hbstate, d_hb_gain);
}
int gtcrn_rate_stream_step_hb_pcm16(gtcrn_model* m, gtcrn_resampler* in, gtcrn_resampler* out, void* d_state, void* d_wstate,
                                    void* d_rstate, const short* d_in, long in_stride, short* d_out, long out_stride,
                                    int nstreams, int nhops, const float* d_gain, const float* d_win, void* d_hbstate,
                                    const float* d_hb_gain, void* stream) {
    return rate_stream_impl<short>("gtcrn_rate_stream_step_hb_pcm16", m, in, out, d_state, d_wstate, d_rstate, d_in, in_stride,
                                   d_out, out_stride, nstreams, nhops, d_win, stream, d_gain, true, d_hbstate, d_hb_gain);
}
int gtcrn_resample_hb(gtcrn_resampler* r, const float* d_wet, long wet_stride, const float* d_dry, long dry_stride,
                      const int* d_lengths, long L, const float* d_x, long x_stride, const int* d_xlengths, long Lx,
                      const float* d_hb_gain, float* d_out, long out_stride, int B, void* stream) {
    const std::string w("gtcrn_resample_hb");
    if (!r || !r->d_taps) return fail(GTCRN_ERR_ARG, w + ": null resampler");
    if (r->fs_in != 16000 || !hb_rate_ok(r->fs_out)) return fail(GTCRN_ERR_ARG, w + ": the resampler must be 16000 -> 24000, 32000 or 48000");
    if (!d_wet || !d_dry || !d_x || !d_hb_gain || !d_out) return fail(GTCRN_ERR_ARG, w + ": null pointer");
    if (B < 1 || L < 1 || Lx < 1) return fail(GTCRN_ERR_ARG, w + ": B, L and Lx must be >= 1");
    const RsDesign& d = r->d;
    const long nout = (L * d.up + d.down - 1) / d.down;
    if (wet_stride < L || dry_stride < L || x_stride < Lx || out_stride < nout)
        return fail(GTCRN_ERR_ARG, w + ": a stride is shorter than its row");
    if (rows_overlap(d_x, x_stride, static_cast<const float*>(d_out), out_stride, Lx < nout ? Lx : nout, B))
        return fail(GTCRN_ERR_ARG, w + ": the x and output rows overlap");
    HIP_TRY(hipSetDevice(r->device));
    LAUNCH_TRY(gtk::launch_resample_hb(d_wet, wet_stride, d_dry, dry_stride, d_lengths, L, d_x, x_stride, d_xlengths, Lx,
                                       d_hb_gain, d_out, out_stride, B, d.up, d.down, d.half, d.ntp, r->d_taps,
                                       static_cast<hipStream_t>(stream)));
    return 0;
}

// ---- packet-sized live streaming: k_packet_in -> the wave step for h hops (nothing when h == 0) -> k_packet_out.
// All geometry is host arithmetic on (fs, n) and the group's phase; the kernels receive the numbers.
namespace {

struct PkGeom {
    int n16 = 0, g = 0, hmax = 0;   // packet at 16 kHz; gcd(n16, 256); the most hops one call steps
    int d_in = 0, d_out = 0;        // the two causal stages' delays in 16 kHz samples (0 at 16 kHz)
    RsDesign in, out;               // (no taps) fs -> 16000 and 16000 -> fs; ntp = 0 at 16 kHz
    // the per-stream state row (floats): [inbound FIFO | outbound FIFO | inbound stage history | outbound stage history]
    int hist_off() const { return 2 * gtk::PK_FIFO + in.ntp; }        // to the outbound stage's history
    long ps_stride() const { return hist_off() + out.ntp; }
};

bool pk_rate_ok(int fs) {
    for (int r : {8000, 16000, 22050, 24000, 32000, 44100, 48000})
        if (fs == r) return true;
    return false;
}
// false: (fs, n) is not a packet this form takes
bool pk_geometry(int fs, int n, PkGeom* p) {
    if (!pk_rate_ok(fs) || n < 1 || n > gtk::PK_MAX16 * 3 || ((long)n * 16000) % fs) return false;
    const long n16 = (long)n * 16000 / fs;
    if (n16 < 1 || n16 > gtk::PK_MAX16) return false;
    p->n16 = (int)n16;
    int a = p->n16, b = 256;
    while (b) { const int t = a % b; a = b; b = t; }
    p->g = a;
    p->hmax = (256 - p->g + p->n16) / 256;
    p->in.ntp = p->out.ntp = 0;
    p->d_in = p->d_out = 0;
    if (fs == 16000) return true;
    rs_design(fs, 16000, &p->in, false);
    rs_design(16000, fs, &p->out, false);
    p->d_in = p->in.half / p->in.down;
    p->d_out = p->out.half / p->out.up;
    // each stage's history comes out of ONE packet, and a staging round of the inbound stage fits its LDS span
    return p->in.ntp <= n && p->out.ntp <= p->n16 && p->out.ntp <= gtk::PK_HIST &&
           ((gtk::PK_TILE - 1) * p->in.down) / p->in.up + p->in.ntp + 1 <= gtk::PK_SPAN;
}
const char* const kPkBad = ": packets are n samples at fs in {8000, 16000, 22050, 24000, 32000, 44100, 48000} with n * 16000 / fs a "
                           "whole number in 1..4096 and, at fs != 16000, no shorter than either filter's history";

// high band on the packet forms: fs in {24000, 32000, 48000} and the latency a whole number of samples at fs
// (always at 32 / 48 kHz; at 24 kHz it needs an even n16).  *lat = latency16 * fs / 16000, *l16 = 512 - g.
bool pk_hb_geometry(int fs, int n, PkGeom* p, int* l16, int* lat) {
    if (!hb_rate_ok(fs) || !pk_geometry(fs, n, p)) return false;
    const long lat16 = 512 - p->g + p->d_in + p->d_out;
    if ((lat16 * fs) % 16000) return false;
    *l16 = 512 - p->g;
    *lat = (int)(lat16 * fs / 16000);
    return *lat <= gtk::PKHB_DELAY && *l16 <= gtk::PKHB_A;
}
// floats per stream of d_hbstate: [l16 | lat], the row rounded up to a multiple of 4 floats
long pk_hb_stride(int l16, int lat) { return ((long)l16 + lat + 3) & ~3L; }
const char* const kPkHbBad = ": the packet high band exists at fs in {24000, 32000, 48000} for packets the packet form takes "
                             "whose latency is a whole number of samples at fs (at 24000: n * 16000 / fs even)";

// the high-band arguments of a packet step (null: the plain call)
struct PkHb {
    void* d_hbstate = nullptr;
    const float* d_gain = nullptr;
};

}  // namespace

struct gtcrn_packet_stream {
    gtcrn_model* m = nullptr;
    gtcrn_resampler *in = nullptr, *out = nullptr;
    int device = 0, fs = 0, n = 0, max_streams = 0;
    PkGeom p;
    int phase = 0;              // (16 kHz samples taken so far) mod 256, the same for every stream of the group
    float* d_a = nullptr;       // hand-offs, max_streams rows of 256 hmax floats: k_packet_in -> wave step,
    float* d_b = nullptr;       // wave step -> k_packet_out
    int last_h = 0, last_n = 0; // hops and streams of the most recent step (gtcrn_packet_stream_debug_handoff)
    const float* d_gain = nullptr;   // the caller's dry gains, max_streams floats (gtcrn_packet_stream_set_dry_gain); NULL: no limit
    // the _slots calls: hmax tables and hmax position arrays of max_streams ints, the rows' old phases, the rounds' counts
    // (k_packet_plan writes them, the later launches of the call read them); d_a / d_b then hold one block per round
    int* d_plan = nullptr;
    int* tab(int r) const { return d_plan + (size_t)r * max_streams; }
    int* pos() const { return d_plan + (size_t)p.hmax * max_streams; }
    int* phi_rec() const { return d_plan + 2 * (size_t)p.hmax * max_streams; }
    int* cnts() const { return phi_rec() + max_streams; }
};

namespace {
// the checks a high-band packet step adds to its plain form's: (fs, n), the two pointers, the state's alignment and rows
// that overlap (the kernel reads x[m - latency] from the input rows while other threads write the output rows)
extern "C++" template <typename S>
int packet_hb_args(const std::string& w, const gtcrn_packet_stream* ps, const PkHb* hb, const S* d_in, long in_stride,
                   const S* d_out, long out_stride, int rows, int* l16, int* lat) {
    PkGeom p;
    if (!pk_hb_geometry(ps->fs, ps->n, &p, l16, lat)) return fail(GTCRN_ERR_ARG, w + kPkHbBad);
    if (!hb->d_hbstate || !hb->d_gain) return fail(GTCRN_ERR_ARG, w + ": null high-band state or gain pointer");
    if (int rc = check_state_alignment(w, {hb->d_hbstate})) return rc;
    if (rows_overlap(d_in, in_stride, d_out, out_stride, (long)ps->n, rows))
        return fail(GTCRN_ERR_ARG, w + ": the input and output rows overlap (the high-band step is not legal in place)");
    return 0;
}
}  // namespace

int gtcrn_packet_stream_n16(int fs, int n) {
    PkGeom p;
    if (!pk_geometry(fs, n, &p)) return fail(GTCRN_ERR_ARG, std::string("gtcrn_packet_stream_n16") + kPkBad);
    return p.n16;
}
int gtcrn_packet_stream_latency16(int fs, int n) {
    PkGeom p;
    if (!pk_geometry(fs, n, &p)) return fail(GTCRN_ERR_ARG, std::string("gtcrn_packet_stream_latency16") + kPkBad);
    return 512 - p.g + p.d_in + p.d_out;
}
size_t gtcrn_packet_stream_state_bytes(int fs, int n) {
    PkGeom p;
    if (!pk_geometry(fs, n, &p)) { (void)fail(GTCRN_ERR_ARG, std::string("gtcrn_packet_stream_state_bytes") + kPkBad); return 0; }
    return sizeof(float) * (size_t)p.ps_stride();
}
int gtcrn_packet_stream_schedule(int fs, int n, int phase, int* next_phase) {
    PkGeom p;
    if (!pk_geometry(fs, n, &p)) return fail(GTCRN_ERR_ARG, std::string("gtcrn_packet_stream_schedule") + kPkBad);
    if (phase < 0 || phase >= 256 || phase % p.g) return fail(GTCRN_ERR_ARG, "gtcrn_packet_stream_schedule: the phase is a multiple of gcd(n16, 256) in 0..255");
    if (next_phase) *next_phase = (phase + p.n16) % 256;
    return (phase + p.n16) / 256;
}

int gtcrn_packet_stream_create(gtcrn_packet_stream** out, gtcrn_model* m, gtcrn_resampler* rs_in, gtcrn_resampler* rs_out, int fs,
                               int n, int max_streams) {
    const std::string w("gtcrn_packet_stream_create");
    if (!out) return fail(GTCRN_ERR_ARG, w + ": null out pointer");
    *out = nullptr;
    PkGeom p;
    if (!pk_geometry(fs, n, &p)) return fail(GTCRN_ERR_ARG, w + kPkBad);
    if (!m) return fail(GTCRN_ERR_ARG, w + ": null model");
    if (max_streams < 1) return fail(GTCRN_ERR_ARG, w + ": max_streams must be >= 1");
    if (fs == 16000) {
        if (rs_in || rs_out) return fail(GTCRN_ERR_ARG, w + ": 16 kHz packets take no resamplers (pass NULL)");
    } else {
        if (!rs_in || !rs_out || !rs_in->d_taps || !rs_out->d_taps) return fail(GTCRN_ERR_ARG, w + ": null resampler");
        if (rs_in->fs_in != fs || rs_in->fs_out != 16000 || rs_out->fs_in != 16000 || rs_out->fs_out != fs)
            return fail(GTCRN_ERR_ARG, w + ": the resamplers must be fs -> 16000 and 16000 -> fs");
        if (rs_in->device != m->device || rs_out->device != m->device)
            return fail(GTCRN_ERR_ARG, w + ": resamplers and model on different devices");
    }
    int rc = check_model(m);
    if (rc) return rc;
    if ((rc = ensure_workspace(m, max_streams, p.hmax, nullptr))) return rc;
    gtcrn_packet_stream* ps = new gtcrn_packet_stream;
    ps->m = m; ps->device = m->device; ps->in = rs_in; ps->out = rs_out; ps->fs = fs; ps->n = n; ps->max_streams = max_streams; ps->p = p;
    const size_t bytes = sizeof(float) * 256 * (size_t)p.hmax * (size_t)max_streams;
    hipError_t e = hipMalloc(&ps->d_a, bytes);
    if (e == hipSuccess) e = hipMalloc(&ps->d_b, bytes);
    if (e == hipSuccess) e = hipMalloc(&ps->d_plan, sizeof(int) * ((2 * (size_t)p.hmax + 1) * (size_t)max_streams + (size_t)p.hmax));
    if (e != hipSuccess) {
        if (ps->d_a) (void)hipFree(ps->d_a);
        if (ps->d_b) (void)hipFree(ps->d_b);
        delete ps;
        return hip_fail(e, "gtcrn_packet_stream_create");
    }
    *out = ps;
    return 0;
}

void gtcrn_packet_stream_destroy(gtcrn_packet_stream* ps) {
    if (!ps) return;
    (void)hipSetDevice(ps->device);
    (void)hipDeviceSynchronize();
    if (ps->d_a) (void)hipFree(ps->d_a);
    if (ps->d_b) (void)hipFree(ps->d_b);
    if (ps->d_plan) (void)hipFree(ps->d_plan);
    delete ps;
}

int gtcrn_packet_stream_phase(const gtcrn_packet_stream* ps) {
    if (!ps) return fail(GTCRN_ERR_ARG, "gtcrn_packet_stream_phase: null handle");
    return ps->phase;
}
int gtcrn_packet_stream_next_hops(const gtcrn_packet_stream* ps) {
    if (!ps) return fail(GTCRN_ERR_ARG, "gtcrn_packet_stream_next_hops: null handle");
    return (ps->phase + ps->p.n16) / 256;
}

int gtcrn_packet_stream_set_dry_gain(gtcrn_packet_stream* ps, const float* d_gain) {
    if (!ps) return fail(GTCRN_ERR_ARG, "gtcrn_packet_stream_set_dry_gain: null handle");
    ps->d_gain = d_gain;
    return 0;
}

int gtcrn_packet_stream_reset(gtcrn_packet_stream* ps, void* d_state, void* d_wstate, void* d_pstate, int nstreams, void* stream) {
    if (!ps) return fail(GTCRN_ERR_ARG, "gtcrn_packet_stream_reset: null handle");
    if (!d_pstate) return fail(GTCRN_ERR_ARG, "gtcrn_packet_stream_reset: null state or nstreams < 1");
    if (nstreams > ps->max_streams) return fail(GTCRN_ERR_ARG, "gtcrn_packet_stream_reset: more streams than the handle was created for");
    if (int rc = gtcrn_wave_stream_reset(ps->m, d_state, d_wstate, nstreams, stream)) return rc;
    // zeros ARE the pre-roll: the FIFO levels follow from the handle's phase, so a stream reset at phase z holds z zeros
    // inbound and 256 - g - z zeros outbound
    HIP_TRY(hipMemsetAsync(d_pstate, 0, sizeof(float) * (size_t)ps->p.ps_stride() * nstreams, (hipStream_t)stream));
    return 0;
}

// ---- packet stream slots (contract: include/gtcrn_micro_hip.h): the phase is one device word per slot, and a call is
// plan -> k_packet_in_slots -> hmax rounds of the indexed wave step -> k_packet_out_slots whatever the phases are.
namespace {
// the slot arguments of a packet step (null: the contiguous call, whose phase is the handle's)
struct PkSlots {
    int* d_phase = nullptr;
    const int* d_slots = nullptr;
    const int* d_count = nullptr;
};
int packet_slots_args(const std::string& w, gtcrn_packet_stream* ps, const void* d_state, const void* d_wstate,
                      const void* d_pstate, const int* d_phase, const int* d_slots, int max_active) {
    if (!ps) return fail(GTCRN_ERR_ARG, w + ": null handle");
    if (!d_state || !d_wstate || !d_pstate || !d_phase || !d_slots) return fail(GTCRN_ERR_ARG, w + ": null pointer");
    if (max_active < 1 || max_active > ps->max_streams)
        return fail(GTCRN_ERR_ARG, w + ": max_active must be >= 1 and at most the handle's max_streams");
    if (reinterpret_cast<uintptr_t>(d_phase) & 3) return fail(GTCRN_ERR_ARG, w + ": the phase words must be 4-byte aligned");
    return check_state_alignment(w, {d_state, d_wstate, d_pstate});
}
}  // namespace

// One packet step, every entry point's: checks, (slots) the plan, the inbound launch, the wave step, the outbound launch.
// nrows: nstreams, or with `sl` the call's max_active.  Each form refuses in the order its contract states.
extern "C++" template <typename S>
static int packet_step(const char* who, gtcrn_packet_stream* ps, void* d_state, void* d_wstate, void* d_pstate, const PkSlots* sl,
                       int nrows, const S* d_in, long in_stride, S* d_out, long out_stride, const float* d_win, void* stream,
                       const PkHb* hb = nullptr) {
    const std::string w(who);
    if (sl) {
        if (int rc0 = packet_slots_args(w, ps, d_state, d_wstate, d_pstate, sl->d_phase, sl->d_slots, nrows)) return rc0;
        if (!d_in || !d_out || !d_win) return fail(GTCRN_ERR_ARG, w + ": null pointer");
    } else {
        if (!ps) return fail(GTCRN_ERR_ARG, w + ": null handle");
        if (!d_state || !d_wstate || !d_pstate || !d_in || !d_out || !d_win) return fail(GTCRN_ERR_ARG, w + ": null pointer");
        if (nrows < 1 || nrows > ps->max_streams)
            return fail(GTCRN_ERR_ARG, w + ": nstreams must be >= 1 and at most the handle's max_streams");
    }
    if (in_stride < ps->n || out_stride < ps->n) return fail(GTCRN_ERR_ARG, w + ": a stride is shorter than its row");
    if (!sl)
        if (int rc0 = check_state_alignment(w, {d_state, d_wstate, d_pstate})) return rc0;
    int l16 = 0, lat = 0;
    if (hb)
        if (int rc0 = packet_hb_args(w, ps, hb, d_in, in_stride, d_out, out_stride, nrows, &l16, &lat)) return rc0;
    gtcrn_model* m = ps->m;
    int rc = check_model(m);
    if (rc) return rc;
    if (hb && m->live.alc)     // (the high band's formulas assume the 16 kHz hand-off at unit gain)
        return fail(GTCRN_ERR_STATE, w + ": the high band does not go together with level control (gtcrn_wave_stream_set_alc)");
    if (sl && (rc = refuse_three_launch_form(w, m))) return rc;           // (before the plan: nothing runs on a refusal)
    hipStream_t s = (hipStream_t)stream;
    const PkGeom& p = ps->p;
    // contiguous: h hops of every row at the handle's phase (possibly none); slots: hmax one-hop rounds of the rows the plan names
    const int phi = sl ? 0 : ps->phase, h = sl ? 1 : (phi + p.n16) / 256, M = ps->max_streams;
    if (h && (rc = ensure_workspace(m, nrows, h, s))) return rc;          // (create reserved max_streams x hmax)
    const gtk::PkPacket pk{ps->n, p.n16, p.g};
    const gtk::PkState st{static_cast<float*>(d_pstate), p.ps_stride(), p.hist_off()};
    gtk::PkRows rw;
    rw.N = nrows;
    if (sl) { rw.rows = gtk::Rows{sl->d_slots, sl->d_count}; rw.phi_rec = ps->phi_rec(); rw.pos = ps->pos(); rw.M = M; }
    else { rw.phi = phi; rw.hand_stride = 256L * h; }
    Timer tm(m, s);
    if (sl) {
        tm.begin(K_PACKET_PLAN);
        LAUNCH_TRY(gtk::launch_packet_plan(sl->d_slots, sl->d_count, nrows, sl->d_phase, p.n16, p.hmax, M, ps->tab(0), ps->pos(),
                                           ps->phi_rec(), ps->cnts(), s));
        tm.end();
    }
    tm.begin(sl ? K_PACKET_IN_SLOTS : K_PACKET_IN);
    LAUNCH_TRY(gtk::launch_packet_in<S>(d_in, in_stride, ps->d_a, pk, st, rw,
                                        {p.in.up, p.in.down, p.in.ntp, ps->in ? ps->in->d_taps : nullptr}, s));
    tm.end();
    if (sl) {
        const long block = 256L * M;
        for (int r = 0; r < p.hmax; ++r) {
            // round r: one hop of the rows that have more than r ready; an empty round's workgroups return at once
            rc = wave_step<float>(who, m, d_state, d_wstate, ps->d_a + block * r, 256, ps->d_b + block * r, 256, nrows, 1, false, 0,
                                  ps->d_gain, d_win, gtk::Rows{ps->tab(r), ps->cnts() + r}, stream);
            if (rc) return rc;
        }
    } else if (h) {
        rc = wave_step<float>("gtcrn_wave_stream_step", m, d_state, d_wstate, ps->d_a, rw.hand_stride, ps->d_b, rw.hand_stride,
                              nrows, h, false, 0, ps->d_gain, d_win, {}, stream);
        if (rc) return rc;
    }
    gtk::PkHighBand band;
    if (hb) band = {ps->d_a, static_cast<float*>(hb->d_hbstate), pk_hb_stride(l16, lat), hb->d_gain, l16, lat};
    tm.begin(sl ? K_PACKET_OUT_SLOTS : K_PACKET_OUT);   // (the high-band kernel is timed in the row of the kernel it stands in for)
    LAUNCH_TRY(gtk::launch_packet_out<S>(ps->d_b, d_in, in_stride, d_out, out_stride, pk, st, rw,
                                         {p.out.up, p.out.down, p.out.ntp, ps->out ? ps->out->d_taps : nullptr}, hb ? &band : nullptr,
                                         s));
    tm.end();
    if (!sl) ps->phase = (phi + p.n16) % 256;
    // (a slot call leaves no contiguous hand-off to copy: gtcrn_packet_stream_debug_handoff is out of scope for it)
    ps->last_h = sl ? 0 : h;
    ps->last_n = sl ? 0 : nrows;
    return 0;
}
// G.711 rows: the same step with the law as the sample type (gtk::g711u / g711a); the strides are in bytes = samples
static int packet_step_g711(const char* who, int law, gtcrn_packet_stream* ps, void* d_state, void* d_wstate, void* d_pstate,
                            const PkSlots* sl, int nrows, const unsigned char* d_in, long in_stride, unsigned char* d_out,
                            long out_stride, const float* d_win, void* stream) {
    if (law != 0 && law != 1) return fail(GTCRN_ERR_ARG, std::string(who) + ": law must be 0 (mu-law) or 1 (A-law)");
    if (law == 0)
        return packet_step<gtk::g711u>(who, ps, d_state, d_wstate, d_pstate, sl, nrows, reinterpret_cast<const gtk::g711u*>(d_in),
                                       in_stride, reinterpret_cast<gtk::g711u*>(d_out), out_stride, d_win, stream);
    return packet_step<gtk::g711a>(who, ps, d_state, d_wstate, d_pstate, sl, nrows, reinterpret_cast<const gtk::g711a*>(d_in),
                                   in_stride, reinterpret_cast<gtk::g711a*>(d_out), out_stride, d_win, stream);
}
int gtcrn_packet_stream_step(gtcrn_packet_stream* ps, void* d_state, void* d_wstate, void* d_pstate, const float* d_in,
                             long in_stride, float* d_out, long out_stride, int nstreams, const float* d_win, void* stream) {
    return packet_step<float>("gtcrn_packet_stream_step", ps, d_state, d_wstate, d_pstate, nullptr, nstreams, d_in, in_stride,
                              d_out, out_stride, d_win, stream);
}
int gtcrn_packet_stream_step_pcm16(gtcrn_packet_stream* ps, void* d_state, void* d_wstate, void* d_pstate, const short* d_in,
                                   long in_stride, short* d_out, long out_stride, int nstreams, const float* d_win, void* stream) {
    return packet_step<short>("gtcrn_packet_stream_step_pcm16", ps, d_state, d_wstate, d_pstate, nullptr, nstreams, d_in,
                              in_stride, d_out, out_stride, d_win, stream);
}
int gtcrn_packet_stream_step_g711(gtcrn_packet_stream* ps, void* d_state, void* d_wstate, void* d_pstate,
                                  const unsigned char* d_in, long in_stride, unsigned char* d_out, long out_stride, int nstreams,
                                  int law, const float* d_win, void* stream) {
    return packet_step_g711("gtcrn_packet_stream_step_g711", law, ps, d_state, d_wstate, d_pstate, nullptr, nstreams, d_in,
                            in_stride, d_out, out_stride, d_win, stream);
}

int gtcrn_packet_stream_reset_slots(gtcrn_packet_stream* ps, void* d_state, void* d_wstate, void* d_pstate, int* d_phase,
                                    const int* d_slots, const int* d_count, int max_active, void* stream) {
    const std::string w("gtcrn_packet_stream_reset_slots");
    if (int rc0 = packet_slots_args(w, ps, d_state, d_wstate, d_pstate, d_phase, d_slots, max_active)) return rc0;
    int rc = check_model(ps->m);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    LAUNCH_TRY(gtk::launch_reset_slots(static_cast<float*>(d_state), static_cast<float*>(d_wstate), d_slots, d_count, max_active, s));
    LAUNCH_TRY(gtk::launch_packet_reset_slots(static_cast<float*>(d_pstate), ps->p.ps_stride(), d_phase, d_slots, d_count,
                                              max_active, s));
    return 0;
}

int gtcrn_packet_stream_step_slots(gtcrn_packet_stream* ps, void* d_state, void* d_wstate, void* d_pstate, int* d_phase,
                                   const int* d_slots, const int* d_count, int max_active, const float* d_in, long in_stride,
                                   float* d_out, long out_stride, const float* d_win, void* stream) {
    const PkSlots sl{d_phase, d_slots, d_count};
    return packet_step<float>("gtcrn_packet_stream_step_slots", ps, d_state, d_wstate, d_pstate, &sl, max_active, d_in, in_stride,
                              d_out, out_stride, d_win, stream);
}
int gtcrn_packet_stream_step_slots_pcm16(gtcrn_packet_stream* ps, void* d_state, void* d_wstate, void* d_pstate, int* d_phase,
                                         const int* d_slots, const int* d_count, int max_active, const short* d_in,
                                         long in_stride, short* d_out, long out_stride, const float* d_win, void* stream) {
    const PkSlots sl{d_phase, d_slots, d_count};
    return packet_step<short>("gtcrn_packet_stream_step_slots_pcm16", ps, d_state, d_wstate, d_pstate, &sl, max_active, d_in,
                              in_stride, d_out, out_stride, d_win, stream);
}
int gtcrn_packet_stream_step_slots_g711(gtcrn_packet_stream* ps, void* d_state, void* d_wstate, void* d_pstate, int* d_phase,
                                        const int* d_slots, const int* d_count, int max_active, const unsigned char* d_in,
                                        long in_stride, unsigned char* d_out, long out_stride, int law, const float* d_win,
                                        void* stream) {
    const PkSlots sl{d_phase, d_slots, d_count};
    return packet_step_g711("gtcrn_packet_stream_step_slots_g711", law, ps, d_state, d_wstate, d_pstate, &sl, max_active, d_in,
                            in_stride, d_out, out_stride, d_win, stream);
}

// ---- high band on the packet forms: the plain launch sequences with k_packet_out_hb / k_packet_out_slots_hb as the last launch
int gtcrn_packet_stream_hb_latency(int fs, int n) {
    PkGeom p;
    int l16 = 0, lat = 0;
    if (!pk_hb_geometry(fs, n, &p, &l16, &lat)) return fail(GTCRN_ERR_ARG, std::string("gtcrn_packet_stream_hb_latency") + kPkHbBad);
    return lat;
}
size_t gtcrn_packet_stream_hb_state_bytes(int fs, int n) {
    PkGeom p;
    int l16 = 0, lat = 0;
    if (!pk_hb_geometry(fs, n, &p, &l16, &lat)) { (void)fail(GTCRN_ERR_ARG, std::string("gtcrn_packet_stream_hb_state_bytes") + kPkHbBad); return 0; }
    return sizeof(float) * (size_t)pk_hb_stride(l16, lat);
}
int gtcrn_packet_stream_hb_reset(gtcrn_packet_stream* ps, void* d_hbstate, int nstreams, void* stream) {
    const std::string w("gtcrn_packet_stream_hb_reset");
    if (!ps) return fail(GTCRN_ERR_ARG, w + ": null handle");
    const size_t bytes = gtcrn_packet_stream_hb_state_bytes(ps->fs, ps->n);
    if (!bytes) return GTCRN_ERR_ARG;
    if (!d_hbstate || nstreams < 1) return fail(GTCRN_ERR_ARG, w + ": null state or nstreams < 1");
    if (nstreams > ps->max_streams) return fail(GTCRN_ERR_ARG, w + ": more streams than the handle was created for");
    if (int rc = check_state_alignment(w, {d_hbstate})) return rc;
    HIP_TRY(hipSetDevice(ps->device));
    HIP_TRY(hipMemsetAsync(d_hbstate, 0, bytes * nstreams, (hipStream_t)stream));
    return 0;
}
int gtcrn_packet_stream_hb_reset_slots(gtcrn_packet_stream* ps, void* d_hbstate, const int* d_slots, const int* d_count,
                                       int max_active, void* stream) {
    const std::string w("gtcrn_packet_stream_hb_reset_slots");
    if (!ps) return fail(GTCRN_ERR_ARG, w + ": null handle");
    const size_t bytes = gtcrn_packet_stream_hb_state_bytes(ps->fs, ps->n);
    if (!bytes) return GTCRN_ERR_ARG;
    if (!d_hbstate || !d_slots) return fail(GTCRN_ERR_ARG, w + ": null pointer");
    if (max_active < 1 || max_active > ps->max_streams)
        return fail(GTCRN_ERR_ARG, w + ": max_active must be >= 1 and at most the handle's max_streams");
    if (int rc = check_state_alignment(w, {d_hbstate})) return rc;
    HIP_TRY(hipSetDevice(ps->device));
    LAUNCH_TRY(gtk::launch_packet_hb_reset_slots(static_cast<float*>(d_hbstate), (long)(bytes / sizeof(float)), d_slots, d_count,
                                                 max_active, (hipStream_t)stream));
    return 0;
}
int gtcrn_packet_stream_step_hb(gtcrn_packet_stream* ps, void* d_state, void* d_wstate, void* d_pstate, const float* d_in,
                                long in_stride, float* d_out, long out_stride, int nstreams, const float* d_win, void* d_hbstate,
                                const float* d_hb_gain, void* stream) {
    const PkHb hb{d_hbstate, d_hb_gain};
    return packet_step<float>("gtcrn_packet_stream_step_hb", ps, d_state, d_wstate, d_pstate, nullptr, nstreams, d_in, in_stride,
                              d_out, out_stride, d_win, stream, &hb);
}
int gtcrn_packet_stream_step_hb_pcm16(gtcrn_packet_stream* ps, void* d_state, void* d_wstate, void* d_pstate, const short* d_in,
                                      long in_stride, short* d_out, long out_stride, int nstreams, const float* d_win,
                                      void* d_hbstate, const float* d_hb_gain, void* stream) {
    const PkHb hb{d_hbstate, d_hb_gain};
    return packet_step<short>("gtcrn_packet_stream_step_hb_pcm16", ps, d_state, d_wstate, d_pstate, nullptr, nstreams, d_in,
                              in_stride, d_out, out_stride, d_win, stream, &hb);
}
int gtcrn_packet_stream_step_slots_hb(gtcrn_packet_stream* ps, void* d_state, void* d_wstate, void* d_pstate, int* d_phase,
                                      const int* d_slots, const int* d_count, int max_active, const float* d_in, long in_stride,
                                      float* d_out, long out_stride, const float* d_win, void* d_hbstate, const float* d_hb_gain,
                                      void* stream) {
    const PkHb hb{d_hbstate, d_hb_gain};
    const PkSlots sl{d_phase, d_slots, d_count};
    return packet_step<float>("gtcrn_packet_stream_step_slots_hb", ps, d_state, d_wstate, d_pstate, &sl, max_active, d_in,
                              in_stride, d_out, out_stride, d_win, stream, &hb);
}
int gtcrn_packet_stream_step_slots_hb_pcm16(gtcrn_packet_stream* ps, void* d_state, void* d_wstate, void* d_pstate, int* d_phase,
                                            const int* d_slots, const int* d_count, int max_active, const short* d_in,
                                            long in_stride, short* d_out, long out_stride, const float* d_win, void* d_hbstate,
                                            const float* d_hb_gain, void* stream) {
    const PkHb hb{d_hbstate, d_hb_gain};
    const PkSlots sl{d_phase, d_slots, d_count};
    return packet_step<short>("gtcrn_packet_stream_step_slots_hb_pcm16", ps, d_state, d_wstate, d_pstate, &sl, max_active, d_in,
                              in_stride, d_out, out_stride, d_win, stream, &hb);
}

long gtcrn_packet_stream_debug_handoff(gtcrn_packet_stream* ps, int which, float* d_dst, long n, void* stream) {
    if (!ps || !d_dst || (which != 0 && which != 1) || n < 1)
        return fail(GTCRN_ERR_ARG, "gtcrn_packet_stream_debug_handoff: null pointer, n < 1 or which not 0 / 1");
    if (n > 256L * ps->last_h * ps->last_n) return fail(GTCRN_ERR_STATE, "gtcrn_packet_stream_debug_handoff: the last step handed over fewer samples");
    int rc = check_model(ps->m);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d_dst, which ? ps->d_b : ps->d_a, sizeof(float) * n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return n;
}

static int state_convert(gtcrn_model* m, void* d_state, int nstreams, float* conv, float* tra,
                         float* const* tcn8, int dir, void* stream) {
    int rc = check_model(m);
    if (rc) return rc;
    if (!d_state || !conv || !tra || !tcn8 || nstreams < 1) return fail(GTCRN_ERR_ARG, "null pointer or nstreams < 1");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(m->d_ptr8, tcn8, sizeof(float*) * 8, hipMemcpyHostToDevice, s));
    LAUNCH_TRY(gtk::launch_state_convert((float*)d_state, nstreams, conv, tra, m->d_ptr8, m->d_pi, dir, s));
    return 0;
}

int gtcrn_stream_import(gtcrn_model* m, void* d_state, int nstreams, const float* d_conv_cache,
                        const float* d_tra_cache, const float* const* d_tcn_cache8, void* stream) {
    return state_convert(m, d_state, nstreams, const_cast<float*>(d_conv_cache), const_cast<float*>(d_tra_cache),
                         const_cast<float* const*>(reinterpret_cast<const float* const*>(d_tcn_cache8)), 0, stream);
}

int gtcrn_stream_export(gtcrn_model* m, const void* d_state, int nstreams, float* d_conv_cache, float* d_tra_cache,
                        float* const* d_tcn_cache8, void* stream) {
    return state_convert(m, const_cast<void*>(d_state), nstreams, d_conv_cache, d_tra_cache, d_tcn_cache8, 1, stream);
}

int gtcrn_stream_conv2d(const float* d_x, const float* d_cache, const float* d_w, const float* d_bias, float* d_y,
                        float* d_cache_out, int B, int Cin, int Cout, int T, int F, int kt, int kf, int dt, int df,
                        int pad_f, int groups, int transposed, void* stream) {
    if (!d_x || !d_w || !d_y) return fail(GTCRN_ERR_ARG, "null pointer");
    // pad_f may be negative: the reference pads by (kF-1)*dF - F_pad, which crops when kF == 1 (convolution.py:243-250)
    if (B < 1 || Cin < 1 || Cout < 1 || T < 1 || F < 1 || kt < 1 || kf < 1 || dt < 1 || df < 1)
        return fail(GTCRN_ERR_ARG, "bad shape");
    const int H = (kt - 1) * dt;
    if (H > 0 && (!d_cache || !d_cache_out)) return fail(GTCRN_ERR_ARG, "a causal kernel taller than 1 needs a cache");
    if (transposed && groups != 1) return fail(GTCRN_ERR_ARG, "transposed form supports groups == 1 only");
    if (!transposed && (groups < 1 || Cin % groups || Cout % groups)) return fail(GTCRN_ERR_ARG, "bad groups");
    const int Fout = transposed ? F - 2 * pad_f + df * (kf - 1) : F + 2 * pad_f - df * (kf - 1);
    if (Fout < 1) return fail(GTCRN_ERR_ARG, "empty output");
    LAUNCH_TRY(gtk::launch_conv2d_causal(d_x, d_cache, d_w, d_bias, d_y, d_cache_out, B, Cin, Cout, T, F, kt, kf, dt,
                                         df, pad_f, groups, transposed, Fout, (hipStream_t)stream));
    return Fout;
}

int gtcrn_debug_enable(gtcrn_model* m, int on) {
    int rc = check_model(m);
    if (rc) return rc;
    m->debug = on != 0;
    m->debug_keep_fused = on == 2;
    return 0;
}

int gtcrn_var_spans_enable(gtcrn_model* m, int on) {
    int rc = check_model(m);
    if (rc) return rc;
    m->var_spans = on != 0;
    return 0;
}

int gtcrn_stream_streams_per_workgroup(int nstreams) {
    if (nstreams < 1) return fail(GTCRN_ERR_ARG, "gtcrn_stream_streams_per_workgroup: nstreams >= 1");
    return stream_wide_pays(nstreams) ? gtk::stream_wide_streams() : 4;
}

int gtcrn_stream_form(gtcrn_model* m, int form) {
    int rc = check_model(m);
    if (rc) return rc;
    if (form < 0 || form > 3)
        return fail(GTCRN_ERR_ARG, "gtcrn_stream_form: 0 (one launch, form by stream count), 1 (three launches), 2 / 3 (one launch: "
                                   "four / seven streams per workgroup)");
    m->stream_form = form;
    return 0;
}

// binary16 bits -> float, exact (the fp16 hand-off records of the int8/fp16 variant, read back for the stage taps)
static float half_bits_to_float(uint16_t h) {
    const int e = (h >> 10) & 31, f = h & 1023;
    float v;
    if (e == 0) v = std::ldexp((float)f, -24);
    else if (e == 31) v = f ? std::numeric_limits<float>::quiet_NaN() : std::numeric_limits<float>::infinity();
    else v = std::ldexp((float)(f | 1024), e - 25);
    return (h & 0x8000) ? -v : v;
}

long gtcrn_debug_tap(gtcrn_model* m, const char* name, int b, float* h_dst, long cap) {
    int rc = check_model(m);
    if (rc) return rc;
    if (!name || !h_dst) return fail(GTCRN_ERR_ARG, "null argument");
    const int B = m->last_B, T = m->last_T;
    if (B < 1 || b < 0 || b >= B) return fail(GTCRN_ERR_ARG, "no forward recorded or batch index out of range");
    if (m->last_fused_stream)
        return fail(GTCRN_ERR_STATE, "the last forward was a single-launch streaming step, which keeps no hand-off "
                                     "tensors: enable debug before the step to run the three-launch form");
    const bool q = m->last_quant;       // the hand-off tensors are fp16 records (HandOff<true>): same element offsets
    if (q && !m->last_quant_taps)
        return fail(GTCRN_ERR_STATE, "the last forward was the int8/fp16 variant without the stage taps: its hand-off tensors "
                                     "are fp16 records, read only after gtcrn_debug_enable(m,1) before the forward");
    const std::string nm(name);
    const long bt = (long)B * T;
    const float* src = nullptr;
    bool handoff = true;                // false: a decoder tap in d_dbg, fp32 in either variant
    int F = 33, perm = -1;
    if (nm == "en0") { src = m->d_en0; F = 65; perm = 0; }
    else if (nm == "en1") { src = m->d_en[0]; perm = 1; }
    else if (nm == "en2") { src = m->d_en[1]; perm = 2; }
    else if (nm == "en3") { src = m->d_en[2]; perm = 3; }
    else if (nm == "en4") { src = m->d_en[3]; perm = 4; }
    else if (nm == "gtcn1") { src = m->d_g1; perm = 4; }
    else if (nm == "gtcn2") {
        if (q)
            return fail(GTCRN_ERR_STATE, "the last forward was the int8/fp16 variant: it stores gtcn2(x) + en4 rounded to "
                                         "fp16, which cannot be un-added -- tap \"sum4\" instead");
        src = m->d_g2; perm = 4;
    }
    else if (nm == "sum4") { src = m->d_g2; perm = 4; }           // gtcn2(x) + en4 as stored: the decoder's first input
    else if (nm == "de0" || nm == "de1" || nm == "de2" || nm == "de3" || nm == "de4") {
        if (!m->debug || !m->d_dbg || m->dbg_cap_bt < bt)
            return fail(GTCRN_ERR_STATE, "decoder taps need gtcrn_debug_enable(m,1) before the forward");
        handoff = false;
        const int j = nm[2] - '0';
        if (j < 3) { src = m->d_dbg + (long)j * bt * 528; perm = 5 + j; }
        else if (j == 3) { src = m->d_dbg + 3 * bt * 528; F = 65; perm = 8; }
        else {
            // de4 is stored as (B,2,T,129) already
            const long nel = 2L * T * 129;
            if (cap < nel) return fail(GTCRN_ERR_ARG, "destination too small");
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(hipMemcpy(h_dst, m->d_dbg + 3 * bt * 528 + bt * 65 * 16 + (long)b * nel, sizeof(float) * nel,
                              hipMemcpyDeviceToHost));
            return nel;
        }
    } else {
        return fail(GTCRN_ERR_ARG, "unknown tap name");
    }
    const long nel = 16L * T * F;
    if (cap < nel) return fail(GTCRN_ERR_ARG, "destination too small");
    std::vector<float> tmp(nel);
    HIP_TRY(hipDeviceSynchronize());
    if (q && handoff) {
        std::vector<uint16_t> hb(nel);
        HIP_TRY(hipMemcpy(hb.data(), reinterpret_cast<const uint16_t*>(src) + (long)b * nel, sizeof(uint16_t) * nel,
                          hipMemcpyDeviceToHost));
        for (long i = 0; i < nel; ++i) tmp[i] = half_bits_to_float(hb[i]);
    } else {
        HIP_TRY(hipMemcpy(tmp.data(), src + (long)b * nel, sizeof(float) * nel, hipMemcpyDeviceToHost));
    }
    if (nm == "gtcn2") {  // stored as gtcn2(x) + en4: recover the stage output for the tap
        std::vector<float> e4(nel);
        HIP_TRY(hipMemcpy(e4.data(), m->d_en[3] + (long)b * nel, sizeof(float) * nel, hipMemcpyDeviceToHost));
        for (long i = 0; i < nel; ++i) tmp[i] -= e4[i];
    }
    const int* pm = m->h_pi.data() + gtl::I_PERM + perm * 16;
    for (int t = 0; t < T; ++t)
        for (int f = 0; f < F; ++f)
            for (int s = 0; s < 16; ++s) h_dst[((long)pm[s] * T + t) * F + f] = tmp[((long)t * F + f) * 16 + s];
    return nel;
}

long gtcrn_debug_stamps(gtcrn_model* m, int kernel, unsigned long long* h_dst, long cap) {
    int rc = check_model(m);
    if (rc) return rc;
    if (kernel < 0 || kernel > 3 || !h_dst) return fail(GTCRN_ERR_ARG, "kernel index 0..3 (encoder, gtcn1, gtcn2, decoder)");
    if (!m->d_stamps) return fail(GTCRN_ERR_STATE, "enable debug before the forward");
    const long n = (long)m->last_B * 16;
    if (cap < n) return fail(GTCRN_ERR_ARG, "destination too small");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h_dst, m->d_stamps + (long)kernel * m->stamps_cap_b * 16, sizeof(unsigned long long) * n,
                      hipMemcpyDeviceToHost));
    return n;
}

namespace {
// the self-tests own their scratch buffers and the device selection: both are put back on EVERY exit path
struct DevBuf {
    float* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
};
struct DeviceScope {
    int prev = -1;
    DeviceScope() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};
}  // namespace

static int pcm16_convert(int device, const void* src, void* dst, long n, int dir, void* stream, const char* who) {
    if (!dst || !src) return fail(GTCRN_ERR_ARG, std::string(who) + ": null pointer");
    if (n <= 0 || (n & 7) || ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15))
        return fail(GTCRN_ERR_ARG, std::string(who) + ": 16-byte aligned device pointers and a sample count that is a multiple of 8");
    DeviceScope scope;              // (a C caller's current device is put back)
    HIP_TRY(hipSetDevice(device));
    LAUNCH_TRY(gtk::launch_pcm16_convert(src, dst, n, dir, static_cast<hipStream_t>(stream)));
    return 0;
}
int gtcrn_pcm16_to_f32(int device, const short* d_pcm, float* d_wave, long n, void* stream) {
    return pcm16_convert(device, d_pcm, d_wave, n, 0, stream, "gtcrn_pcm16_to_f32");
}
int gtcrn_f32_to_pcm16(int device, const float* d_wave, short* d_pcm, long n, void* stream) {
    return pcm16_convert(device, d_wave, d_pcm, n, 1, stream, "gtcrn_f32_to_pcm16");
}

static int g711_convert(int device, int law, const void* src, void* dst, long n, int dir, void* stream, const char* who) {
    if (law != 0 && law != 1) return fail(GTCRN_ERR_ARG, std::string(who) + ": law must be 0 (mu-law) or 1 (A-law)");
    if (!dst || !src) return fail(GTCRN_ERR_ARG, std::string(who) + ": null pointer");
    if (n <= 0 || (n & 15) || ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15))
        return fail(GTCRN_ERR_ARG, std::string(who) + ": 16-byte aligned device pointers and a sample count that is a multiple of 16");
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    LAUNCH_TRY(gtk::launch_g711_convert(src, dst, n, law, dir, static_cast<hipStream_t>(stream)));
    return 0;
}
int gtcrn_g711_to_f32(int device, int law, const unsigned char* d_codes, float* d_wave, long n, void* stream) {
    return g711_convert(device, law, d_codes, d_wave, n, 0, stream, "gtcrn_g711_to_f32");
}
int gtcrn_f32_to_g711(int device, int law, const float* d_wave, unsigned char* d_codes, long n, void* stream) {
    return g711_convert(device, law, d_wave, d_codes, n, 1, stream, "gtcrn_f32_to_g711");
}
// host only: the kernels' own decode / encode functions (kernels.h), so the table and the map ARE what the device computes
int gtcrn_g711_decode_table(int law, short* h_table) {
    if ((law != 0 && law != 1) || !h_table) return fail(GTCRN_ERR_ARG, "gtcrn_g711_decode_table: law must be 0 or 1 and the table not NULL");
    for (unsigned c = 0; c < 256; ++c) h_table[c] = (short)gtk::g711_decode(law, c);
    return 0;
}
int gtcrn_g711_encode_pcm16(int law, int p) {
    if (law != 0 && law != 1) return fail(GTCRN_ERR_ARG, "gtcrn_g711_encode_pcm16: law must be 0 (mu-law) or 1 (A-law)");
    if (p < -32768 || p > 32767) return fail(GTCRN_ERR_ARG, "gtcrn_g711_encode_pcm16: p outside the int16 range");
    return (int)gtk::g711_encode(law, p);
}

int gtcrn_selftest_mfma(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(GTCRN_ERR_DEVICE, "no HIP device");
    DeviceScope restore;
    HIP_TRY(hipSetDevice(device));
    float hA[64], hB[64], hC[256], hD[256], ref[256];
    for (int i = 0; i < 16; ++i)
        for (int k = 0; k < 4; ++k) hA[i * 4 + k] = (float)(1 + i * 5 + k * 3);       // asymmetric integers
    for (int k = 0; k < 4; ++k)
        for (int j = 0; j < 16; ++j) hB[k * 16 + j] = (float)(2 + k * 7 - j * 2 + (j * j) % 5);
    for (int i = 0; i < 256; ++i) hC[i] = (float)((i * 37) % 101 - 50);
    for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j) {
            float s = hC[i * 16 + j];
            for (int k = 0; k < 4; ++k) s += hA[i * 4 + k] * hB[k * 16 + j];
            ref[i * 16 + j] = s;
        }
    DevBuf bA, bB, bC, bD;
    HIP_TRY(bA.alloc(sizeof(hA))); HIP_TRY(bB.alloc(sizeof(hB)));
    HIP_TRY(bC.alloc(sizeof(hC))); HIP_TRY(bD.alloc(sizeof(hD)));
    float *dA = bA.p, *dB = bB.p, *dC = bC.p, *dD = bD.p;
    HIP_TRY(hipMemcpy(dA, hA, sizeof(hA), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dB, hB, sizeof(hB), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dC, hC, sizeof(hC), hipMemcpyHostToDevice));
    LAUNCH_TRY(gtk::launch_selftest(dA, dB, dC, dD, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(hD, dD, sizeof(hD), hipMemcpyDeviceToHost));
    int bad = 0;
    for (int i = 0; i < 256; ++i) bad += hD[i] != ref[i];
    if (bad) return fail(GTCRN_ERR_DEVICE, "MFMA 16x16x4 f32 lane map differs from the assumed one (" +
                                               std::to_string(bad) + " of 256 elements)");
    return 0;
}

int gtcrn_selftest_split3(int device, const float* h_x, long n, float* h_planes, float* h_joined, const float* h_A,
                          const float* h_B, float* h_D) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(GTCRN_ERR_DEVICE, "no HIP device");
    if (!h_x || !h_planes || !h_joined || n < 4 || (n & 3)) return fail(GTCRN_ERR_ARG, "n must be a positive multiple of 4");
    if ((h_A || h_B || h_D) && !(h_A && h_B && h_D)) return fail(GTCRN_ERR_ARG, "A, B and D come together");
    DeviceScope restore;
    HIP_TRY(hipSetDevice(device));
    DevBuf bx, bp, bj, bm;             // (freed on every exit path, ADVICE r4: a failing call leaked all four)
    HIP_TRY(bx.alloc(sizeof(float) * n));
    HIP_TRY(bp.alloc(sizeof(float) * 3 * n));
    HIP_TRY(bj.alloc(sizeof(float) * n));
    HIP_TRY(bm.alloc(sizeof(float) * (512 + 512 + 256)));
    float *dx = bx.p, *dp = bp.p, *dj = bj.p, *dm = bm.p;
    HIP_TRY(hipMemcpy(dx, h_x, sizeof(float) * n, hipMemcpyHostToDevice));
    if (h_A) {
        HIP_TRY(hipMemcpy(dm, h_A, sizeof(float) * 512, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dm + 512, h_B, sizeof(float) * 512, hipMemcpyHostToDevice));
    }
    LAUNCH_TRY(gtk::launch_selftest_split3(dx, n, dp, dj, h_A ? dm : nullptr, dm + 512, dm + 1024, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h_planes, dp, sizeof(float) * 3 * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_joined, dj, sizeof(float) * n, hipMemcpyDeviceToHost));
    if (h_D) HIP_TRY(hipMemcpy(h_D, dm + 1024, sizeof(float) * 256, hipMemcpyDeviceToHost));
    return 0;
}

int gtcrn_timing_enable(gtcrn_model* m, int on) {
    int rc = check_model(m);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    for (auto& t : m->timings) m->ev_pool.push_back(t);
    m->timings.clear();
    m->timing = on != 0;
    m->timing_only = on >= 2 ? on - 2 : -1;
    if (m->timing_only >= kNumKernels) return fail(GTCRN_ERR_ARG, "gtcrn_timing_enable: no such kernel index");
    return 0;
}

int gtcrn_timing_kernels(void) { return kNumKernels; }

int gtcrn_timing_read(gtcrn_model* m, int idx, char* name, int name_cap, float* ms, int* launches) {
    if (idx < 0) {   // name query only (no model needed): idx = -1 - k
        const int k = -1 - idx;
        if (k >= kNumKernels || !name || name_cap < 1) return fail(GTCRN_ERR_ARG, "timing index out of range");
        std::strncpy(name, kKernelNames[k], name_cap - 1);
        name[name_cap - 1] = 0;
        if (ms) *ms = 0.f;
        if (launches) *launches = 0;
        return 0;
    }
    int rc = check_model(m);
    if (rc) return rc;
    if (idx < 0 || idx >= kNumKernels || !ms) return fail(GTCRN_ERR_ARG, "timing index out of range");
    double sum = 0.0;
    int n = 0;
    for (auto& t : m->timings)
        if (t.kernel == idx) {
            float v = 0.f;
            HIP_TRY(hipEventSynchronize(t.b));
            HIP_TRY(hipEventElapsedTime(&v, t.a, t.b));
            sum += v;
            ++n;
        }
    *ms = n ? (float)(sum / n) : 0.f;
    if (launches) *launches = n;
    if (name && name_cap > 0) {
        std::strncpy(name, kKernelNames[idx], name_cap - 1);
        name[name_cap - 1] = 0;
    }
    return 0;
}

}  // extern "C"
