// plc_host.cpp -- the "packet loss concealment" section of include/gtcrn_micro_hip.h: the parameter words, argument checks, the
// launches and the host twins gtcrn_plc_rows_host / _pcm16_host / _g711_host, which run plc.h's own functions -- the ones plc.hip
// compiles for the device -- row by row on host pointers.  Compiled with -ffp-contract=off like plc.hip.
#include "../../include/gtcrn_micro_hip.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "plc.h"

extern "C" void gtcrn_set_error_(const char* msg);   // api.cpp: thread-local last error

static_assert(GTCRN_PLC_MAX_HISTORY == gtl::MAX_LH, "the header states the longest history");
static_assert(sizeof(gtl::Record) == 16 && sizeof(gtl::Prm) == 32, "a record is 16 bytes, the parameter words are 8 ints");

namespace {

int pfail(const std::string& m) {
    gtcrn_set_error_(m.c_str());
    return GTCRN_ERR_ARG;
}

constexpr int RATES[] = {8000, 16000, 22050, 24000, 32000, 44100, 48000};

// the checks the device and the host entries share; fills `a`
int plc_args(const std::string& w, int kind, void* x, long stride, int M, int n, const int* slots, const int* lost, const int* count,
             short* hist, long hist_stride, int* rec, int S, const int* params, int law, gtl::PlcArgs* a) {
    const uintptr_t elem = kind == 0 ? 4 : (kind == 1 ? 2 : 1);
    if (M < 0 || S < 0) return pfail(w + ": a negative count");
    if (n < 1 || n > gtl::MAX_N) return pfail(w + ": n must lie in 1 .. 1024");
    if (!lost || !hist || !rec || !params || (M > 0 && !x)) return pfail(w + ": null pointer");
    if (stride < n) return pfail(w + ": the stride is shorter than a row");
    if (hist_stride < 1) return pfail(w + ": hist_stride must be positive");
    if (kind == 2 && law != 0 && law != 1) return pfail(w + ": law must be 0 (mu-law) or 1 (A-law)");
    const auto at = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    if (at(x) & (elem - 1) || at(hist) & 1 || (at(slots) | at(lost) | at(count)) & 3 || (at(rec) | at(params)) & 15)
        return pfail(w + ": misaligned pointer (rows by their sample, histories by 2 bytes, records and parameters by 16 bytes)");
    a->x = x; a->stride = stride; a->hist_stride = hist_stride;
    a->slots = slots; a->lost = lost; a->count = count;
    a->hist = hist;
    a->rec = reinterpret_cast<gtl::Record*>(rec);
    a->params = params;
    a->M = M; a->n = n; a->S = S; a->law = law;
    return 0;
}

// One row on the host: the kernel's cases in the same order, the 64 lanes as a loop.
template <class T>
void plc_row(const gtl::PlcArgs& a, int row) {
    using namespace gtl;
    const int slot = slot_of(a.slots, row, a.S);
    if (slot < 0) return;
    const Prm prm = prm_of(a.params);
    if (!prm_ok(prm, a.hist_stride)) return;
    const int Lh = hist_len(prm), n = a.n;
    const Record r = record_of(a.rec[slot], prm);
    T* x = static_cast<T*>(a.x) + (long)row * a.stride;
    short* ring = a.hist + (long)slot * a.hist_stride;
    const bool lost = a.lost[row] != 0;
    const int keep = first_kept(n, Lh), pos = (r.pos + n) % Lh;

    if (!lost && r.erased == 0) {
        for (int j = keep; j < n; ++j) ring[ring_at(r.pos, j, Lh)] = (short)sample_in(x[j], a.law);
        a.rec[slot].pos = pos;
        return;
    }
    std::vector<short> h(Lh);
    for (int j = 0; j < Lh; ++j) h[j] = ring[ring_at(r.pos, j, Lh)];
    const bool begins = lost && r.erased == 0;
    int P = r.lag;
    if (begins) {
        std::vector<short> an(Lh);
        int m = 0;
        for (int j = 0; j < Lh; ++j) m = m > abs16(h[j]) ? m : abs16(h[j]);
        const int sh = analysis_shift(m);
        for (int j = 0; j < Lh; ++j) an[j] = (short)(h[j] >> sh);
        double bs = 0.0;
        int bp = NO_LAG;
        for (int p = prm.pmin; p <= prm.pmax; p += prm.D) {
            const double s = score_at(an.data(), Lh, p, prm.D, prm.W);
            if (better(s, p, bs, bp)) { bs = s; bp = p; }
        }
        if (bp == NO_LAG) {
            P = prm.pmax;
        } else {
            const int p0 = bp, lo = refine_lo(p0, prm), hi = refine_hi(p0, prm);
            bs = 0.0;
            bp = NO_LAG;
            for (int p = lo; p <= hi; ++p) {
                const double s = score_at(an.data(), Lh, p, 1, prm.W);
                if (better(s, p, bs, bp)) { bs = s; bp = p; }
            }
            P = bp == NO_LAG ? p0 : bp;
        }
    }
    if (lost) {
        for (int j = 0; j < n; ++j) {
            const int s = synth(h.data(), Lh, P, j);
            sample_out(x + j, attenuated(s, r.erased + j, prm), a.law);
            if (j >= keep) ring[ring_at(r.pos, j, Lh)] = (short)s;
        }
        a.rec[slot] = {pos, P, saturate_erased(r.erased, n, prm), events_next(r.events, begins)};
    } else {
        const int f = prm.F < n ? prm.F : n;
        for (int j = 0; j < n; ++j) {
            if (j < f) recover(x + j, attenuated(synth(h.data(), Lh, P, j), r.erased + j, prm), recover_ramp(j, f), a.law);
            if (j >= keep) ring[ring_at(r.pos, j, Lh)] = (short)sample_in(x[j], a.law);
        }
        a.rec[slot] = {pos, P, 0, r.events};
    }
}

int plc_device(const char* name, int kind, void* x, long stride, int M, int n, const int* slots, const int* lost, const int* count,
               short* hist, long hist_stride, int* rec, int S, const int* params, int law, void* stream) {
    const std::string w(name);
    gtl::PlcArgs a;
    const int rc = plc_args(w, kind, x, stride, M, n, slots, lost, count, hist, hist_stride, rec, S, params, law, &a);
    if (rc != 0) return rc;
    const int e = gtl::launch_plc(a, kind, static_cast<hipStream_t>(stream));
    if (e != 0) {
        gtcrn_set_error_((w + ": " + hipGetErrorString(static_cast<hipError_t>(e))).c_str());
        return GTCRN_ERR_HIP;
    }
    return 0;
}

template <class T>
int plc_host(const char* name, int kind, T* x, long stride, int M, int n, const int* slots, const int* lost, const int* count,
             short* hist, long hist_stride, int* rec, int S, const int* params, int law) {
    gtl::PlcArgs a;
    const int rc = plc_args(name, kind, x, stride, M, n, slots, lost, count, hist, hist_stride, rec, S, params, law, &a);
    if (rc != 0) return rc;
    const int live = gtl::live_rows(M, count);
    for (int row = 0; row < live; ++row) plc_row<T>(a, row);
    return 0;
}

}  // namespace

int gtcrn_plc_params_host(const gtcrn_plc_config* c, int* out8) {
    const std::string w("gtcrn_plc_params_host");
    if (!c || !out8) return pfail(w + ": null pointer");
    bool known = false;
    for (int r : RATES) known = known || r == c->fs;
    if (!known) return pfail(w + ": fs must be one of 8000, 16000, 22050, 24000, 32000, 44100, 48000");
    if (c->hold_ms < 0 || c->hold_ms > gtl::MAX_FADE_MS) return pfail(w + ": hold_ms must lie in 0 .. 200");
    if (c->fade_ms < 1 || c->fade_ms > gtl::MAX_FADE_MS) return pfail(w + ": fade_ms must lie in 1 .. 200");
    if (c->recover_ms < 0 || c->recover_ms > gtl::MAX_FADE_MS) return pfail(w + ": recover_ms must lie in 0 .. 200");
    const int fs = c->fs, F = c->recover_ms * fs / 1000;
    const gtl::Prm p = {fs / 200, fs * 15 / 1000, fs / 50, fs / 8000 > 1 ? fs / 8000 : 1, c->hold_ms * fs / 1000, c->fade_ms * fs / 1000,
                        F > 1 ? F : 1, fs};
    const int words[8] = {p.pmin, p.pmax, p.W, p.D, p.T0, p.T1, p.F, p.fs};
    for (int i = 0; i < 8; ++i) out8[i] = words[i];
    return 0;
}

int gtcrn_plc_rows(float* d_x, long stride, int M, int n, const int* d_slots, const int* d_lost, const int* d_count, short* d_hist,
                   long hist_stride, int* d_rec, int S, const int* d_params, void* stream) {
    return plc_device("gtcrn_plc_rows", 0, d_x, stride, M, n, d_slots, d_lost, d_count, d_hist, hist_stride, d_rec, S, d_params, 0, stream);
}

int gtcrn_plc_rows_pcm16(short* d_x, long stride, int M, int n, const int* d_slots, const int* d_lost, const int* d_count,
                         short* d_hist, long hist_stride, int* d_rec, int S, const int* d_params, void* stream) {
    return plc_device("gtcrn_plc_rows_pcm16", 1, d_x, stride, M, n, d_slots, d_lost, d_count, d_hist, hist_stride, d_rec, S, d_params, 0,
                      stream);
}

int gtcrn_plc_rows_g711(unsigned char* d_x, long stride, int M, int n, const int* d_slots, const int* d_lost, const int* d_count,
                        short* d_hist, long hist_stride, int* d_rec, int S, const int* d_params, int law, void* stream) {
    return plc_device("gtcrn_plc_rows_g711", 2, d_x, stride, M, n, d_slots, d_lost, d_count, d_hist, hist_stride, d_rec, S, d_params, law,
                      stream);
}

int gtcrn_plc_reset(short* d_hist, long hist_stride, int* d_rec, int S, const int* d_params, const int* d_slots, int M,
                    const int* d_count, void* stream) {
    const std::string w("gtcrn_plc_reset");
    if (M < 0 || S < 0) return pfail(w + ": a negative count");
    if (!d_hist || !d_rec || !d_params) return pfail(w + ": null pointer");
    if (hist_stride < 1) return pfail(w + ": hist_stride must be positive");
    const auto at = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    if (at(d_hist) & 1 || (at(d_slots) | at(d_count)) & 3 || (at(d_rec) | at(d_params)) & 15)
        return pfail(w + ": misaligned pointer (histories by 2 bytes, records and parameters by 16 bytes)");
    const int e = gtl::launch_plc_reset(d_hist, hist_stride, reinterpret_cast<gtl::Record*>(d_rec), S, d_params, d_slots, M, d_count,
                                        static_cast<hipStream_t>(stream));
    if (e != 0) {
        gtcrn_set_error_((w + ": " + hipGetErrorString(static_cast<hipError_t>(e))).c_str());
        return GTCRN_ERR_HIP;
    }
    return 0;
}

int gtcrn_plc_rows_host(float* h_x, long stride, int M, int n, const int* h_slots, const int* h_lost, const int* h_count, short* h_hist,
                        long hist_stride, int* h_rec, int S, const int* h_params) {
    return plc_host<float>("gtcrn_plc_rows_host", 0, h_x, stride, M, n, h_slots, h_lost, h_count, h_hist, hist_stride, h_rec, S, h_params, 0);
}

int gtcrn_plc_rows_pcm16_host(short* h_x, long stride, int M, int n, const int* h_slots, const int* h_lost, const int* h_count,
                              short* h_hist, long hist_stride, int* h_rec, int S, const int* h_params) {
    return plc_host<short>("gtcrn_plc_rows_pcm16_host", 1, h_x, stride, M, n, h_slots, h_lost, h_count, h_hist, hist_stride, h_rec, S,
                           h_params, 0);
}

int gtcrn_plc_rows_g711_host(unsigned char* h_x, long stride, int M, int n, const int* h_slots, const int* h_lost, const int* h_count,
                             short* h_hist, long hist_stride, int* h_rec, int S, const int* h_params, int law) {
    return plc_host<unsigned char>("gtcrn_plc_rows_g711_host", 2, h_x, stride, M, n, h_slots, h_lost, h_count, h_hist, hist_stride, h_rec,
                                   S, h_params, law);
}
