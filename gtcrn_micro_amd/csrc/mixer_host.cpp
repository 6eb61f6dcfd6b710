// mixer_host.cpp -- the "conference rooms" section of include/gtcrn_micro_hip.h: the parameter words, argument checks, the launch
// and the host twins gtcrn_mix_rooms_host / gtcrn_mix_rooms_pcm16_host, which run mixer.h's own functions -- the ones mixer.hip
// compiles for the device -- room by room on host pointers.  Compiled with -ffp-contract=off like mixer.hip.
#include "../../include/gtcrn_micro_hip.h"

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "mixer.h"

extern "C" void gtcrn_set_error_(const char* msg);   // api.cpp: thread-local last error

static_assert(GTCRN_MIX_MAX_ROOM == gtm::MAX_ROOM, "the header states the largest room");
static_assert(sizeof(gtm::Seat) == 16 && sizeof(gtm::Record) == 16, "a seat and a record are 16 bytes each");

namespace {

int mfail(const std::string& m) {
    gtcrn_set_error_(m.c_str());
    return GTCRN_ERR_ARG;
}

// the checks the device and the host entries share; fills `a`
int mix_args(const std::string& w, int pcm, const void* in, long in_stride, int n_in, void* out, long out_stride, int n_out, int n,
             const int* room_start, const int* seats, int n_seats, int R, const int* nrooms, float* rec, int n_rec,
             const float* params, const float* voice, long voice_stride, gtm::MixArgs* a) {
    const uintptr_t elem = pcm ? 2 : 4;
    if (n_in < 0 || n_out < 0 || n_seats < 0 || R < 0 || n_rec < 0) return mfail(w + ": a negative count");
    if (n < 1 || n > gtm::MAX_N) return mfail(w + ": n must lie in 1 .. 1024");
    if (!room_start || !seats || !rec || !params || (n_in > 0 && !in) || (n_out > 0 && !out)) return mfail(w + ": null pointer");
    if (in_stride < n || out_stride < n) return mfail(w + ": a stride is shorter than its row");
    if (voice && voice_stride < 1) return mfail(w + ": voice_stride must be positive");
    const auto at = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    if ((at(in) | at(out)) & (elem - 1) || (at(room_start) | at(nrooms) | at(voice)) & 3 || (at(seats) | at(rec) | at(params)) & 15)
        return mfail(w + ": misaligned pointer (rows by their sample, seats, records and parameters by 16 bytes)");
    if (n_in > 0 && n_out > 0) {
        const uintptr_t i0 = at(in), i1 = i0 + ((uintptr_t)(n_in - 1) * (uintptr_t)in_stride + (uintptr_t)n) * elem;
        const uintptr_t o0 = at(out), o1 = o0 + ((uintptr_t)(n_out - 1) * (uintptr_t)out_stride + (uintptr_t)n) * elem;
        if (i0 < o1 && o0 < i1) return mfail(w + ": the input rows overlap the output rows");
    }
    a->in = in; a->out = out;
    a->in_stride = in_stride; a->out_stride = out_stride; a->voice_stride = voice ? voice_stride : 0;
    a->room_start = room_start;
    a->seats = reinterpret_cast<const gtm::Seat*>(seats);
    a->nrooms = nrooms;
    a->rec = reinterpret_cast<gtm::Record*>(rec);
    a->params = params;
    a->voice = voice;
    a->n_in = n_in; a->n_out = n_out; a->n = n; a->R = R; a->n_seats = n_seats; a->n_rec = n_rec;
    a->vec = (n & 3) == 0 && (out_stride & 3) == 0 && (at(out) & (4 * elem - 1)) == 0;
    return 0;
}

// One room on the host: the kernel's phases in the same order, the 64 lanes as a loop.
template <class T>
void mix_room(const gtm::MixArgs& a, int s0, int ns) {
    using namespace gtm;
    const int n = a.n;
    const Params prm = params_of(a.params, n);
    const T* in = static_cast<const T*>(a.in);
    T* out = static_cast<T*>(a.out);
    std::vector<Seat> seat(ns);
    std::vector<float> key(ns), level(ns);
    std::vector<int> flags(ns);
    for (int p = 0; p < ns; ++p) {                           // steps 1 - 5
        const Seat st = seat[p] = seat_of(a.seats[s0 + p], a.n_in, a.n_out, a.n_rec);
        float v[LANES] = {0.0f};
        if (st.in_row >= 0) {
            for (int l = 0; l < LANES; ++l) v[l] = lane_energy(in + (long)st.in_row * a.in_stride, n, l);
            for (int d = 1; d < LANES; d <<= 1) {
                float t[LANES];
                for (int l = 0; l < LANES; ++l) t[l] = v[l] + v[l ^ d];
                for (int l = 0; l < LANES; ++l) v[l] = t[l];
            }
        }
        SeatState ss = {-1.0f, 0.0f, 0};
        if (st.rec >= 0) {
            const bool voiced = a.voice ? a.voice[(long)st.rec * a.voice_stride] != 0.0f : false;
            ss = seat_state(st.in_row >= 0, v[0], a.rec[st.rec], a.voice != nullptr, voiced, prm);
        }
        key[p] = ss.key; level[p] = ss.level; flags[p] = ss.flags;
    }
    for (int round = 0; round < prm.K; ++round) {            // step 6
        float bk = -1.0f;
        int bp = MAX_ROOM;
        for (int p = 0; p < ns; ++p)
            if (key[p] > 0.0f && !(flags[p] & F_T) && goes_before(key[p], p, bk, bp)) { bk = key[p]; bp = p; }
        if (!(bk > 0.0f)) break;
        flags[bp] |= F_T;
    }
    int con[MAX_CONTRIB], nc = 0;
    for (int p = 0; p < ns; ++p)
        if (contributes(flags[p]) && nc < MAX_CONTRIB) {
            con[nc++] = p;
            flags[p] |= nc << F_CSHIFT;
        }
    for (int p = 0; p < ns; ++p)                             // step 9
        if (seat[p].rec >= 0) a.rec[seat[p].rec] = record_next(a.rec[seat[p].rec], flags[p], level[p]);
    const float nf = (float)n;                               // steps 7 and 8
    std::vector<float> stage((size_t)STAGE_ROWS * n);
    for (int c = 0; c < nc; ++c)
        for (int i = 0; i < n; ++i) stage[(size_t)c * n + i] = gained(in + (long)seat[con[c]].in_row * a.in_stride, flags[con[c]], i, nf);
    for (int i = 0; i < n; ++i) {
        float acc = 0.0f;
        for (int c = 0; c < nc; ++c) acc = acc + stage[(size_t)c * n + i];
        stage[(size_t)MAX_CONTRIB * n + i] = acc;
    }
    for (int p = 0; p < ns; ++p) {
        if (seat[p].out_row < 0) continue;
        const int me = (flags[p] >> F_CSHIFT) - 1;
        T* dst = out + (long)seat[p].out_row * a.out_stride;
        for (int i = 0; i < n; ++i) {
            float acc = stage[(size_t)MAX_CONTRIB * n + i];
            if (me >= 0) {
                acc = 0.0f;
                for (int c = 0; c < nc; ++c)
                    if (c != me) acc = acc + stage[(size_t)c * n + i];
            }
            put(dst + i, acc);
        }
    }
}

template <class T>
void mix_host(const gtm::MixArgs& a) {
    const int live = gtm::live_rooms(a.R, a.nrooms);
    for (int r = 0; r < live; ++r) {
        const int s0 = a.room_start[r], s1 = a.room_start[r + 1];
        if (gtm::room_ok(s0, s1, a.n_seats) && s1 > s0) mix_room<T>(a, s0, s1 - s0);
    }
}

int mix_device(const char* name, int pcm, const void* in, long in_stride, int n_in, void* out, long out_stride, int n_out, int n,
               const int* room_start, const int* seats, int n_seats, int R, const int* nrooms, float* rec, int n_rec,
               const float* params, const float* voice, long voice_stride, void* stream) {
    const std::string w(name);
    gtm::MixArgs a;
    const int rc = mix_args(w, pcm, in, in_stride, n_in, out, out_stride, n_out, n, room_start, seats, n_seats, R, nrooms, rec, n_rec,
                            params, voice, voice_stride, &a);
    if (rc != 0) return rc;
    const int e = gtm::launch_mix(a, pcm, static_cast<hipStream_t>(stream));
    if (e != 0) {
        gtcrn_set_error_((w + ": " + hipGetErrorString(static_cast<hipError_t>(e))).c_str());
        return GTCRN_ERR_HIP;
    }
    return 0;
}

}  // namespace

int gtcrn_mix_params_host(const gtcrn_mix_config* c, float* out8) {
    const std::string w("gtcrn_mix_params_host");
    if (!c || !out8) return mfail(w + ": null pointer");
    if (!std::isfinite(c->floor_dbov) || !std::isfinite(c->alpha) || !std::isfinite(c->incumbent_db))
        return mfail(w + ": a field is not finite");
    if (c->k < 1 || c->k > gtm::MAX_K) return mfail(w + ": k must lie in 1 .. 8");
    if (c->alpha < 0 || c->alpha > 1) return mfail(w + ": alpha outside [0, 1]");
    if (c->incumbent_db < 0) return mfail(w + ": incumbent_db is negative");
    const auto fin = [](double x) { return (float)std::min(x, (double)FLT_MAX); };
    for (int i = 0; i < 8; ++i) out8[i] = 0.0f;
    out8[0] = (float)c->k;
    out8[1] = fin(std::pow(10.0, c->floor_dbov / 10.0));
    out8[2] = (float)c->alpha;
    out8[3] = fin(std::pow(10.0, c->incumbent_db / 10.0));
    return 0;
}

int gtcrn_mix_rooms(const float* d_in, long in_stride, int n_in, float* d_out, long out_stride, int n_out, int n,
                    const int* d_room_start, const int* d_seats, int n_seats, int R, const int* d_nrooms, float* d_rec, int n_rec,
                    const float* d_params, const float* d_voice, long voice_stride, void* stream) {
    return mix_device("gtcrn_mix_rooms", 0, d_in, in_stride, n_in, d_out, out_stride, n_out, n, d_room_start, d_seats, n_seats, R,
                      d_nrooms, d_rec, n_rec, d_params, d_voice, voice_stride, stream);
}

int gtcrn_mix_rooms_pcm16(const short* d_in, long in_stride, int n_in, short* d_out, long out_stride, int n_out, int n,
                          const int* d_room_start, const int* d_seats, int n_seats, int R, const int* d_nrooms, float* d_rec,
                          int n_rec, const float* d_params, const float* d_voice, long voice_stride, void* stream) {
    return mix_device("gtcrn_mix_rooms_pcm16", 1, d_in, in_stride, n_in, d_out, out_stride, n_out, n, d_room_start, d_seats, n_seats,
                      R, d_nrooms, d_rec, n_rec, d_params, d_voice, voice_stride, stream);
}

int gtcrn_mix_rooms_host(const float* h_in, long in_stride, int n_in, float* h_out, long out_stride, int n_out, int n,
                         const int* h_room_start, const int* h_seats, int n_seats, int R, const int* h_nrooms, float* h_rec,
                         int n_rec, const float* h_params, const float* h_voice, long voice_stride) {
    gtm::MixArgs a;
    const int rc = mix_args("gtcrn_mix_rooms_host", 0, h_in, in_stride, n_in, h_out, out_stride, n_out, n, h_room_start, h_seats,
                            n_seats, R, h_nrooms, h_rec, n_rec, h_params, h_voice, voice_stride, &a);
    if (rc != 0) return rc;
    mix_host<float>(a);
    return 0;
}

int gtcrn_mix_rooms_pcm16_host(const short* h_in, long in_stride, int n_in, short* h_out, long out_stride, int n_out, int n,
                               const int* h_room_start, const int* h_seats, int n_seats, int R, const int* h_nrooms, float* h_rec,
                               int n_rec, const float* h_params, const float* h_voice, long voice_stride) {
    gtm::MixArgs a;
    const int rc = mix_args("gtcrn_mix_rooms_pcm16_host", 1, h_in, in_stride, n_in, h_out, out_stride, n_out, n, h_room_start,
                            h_seats, n_seats, R, h_nrooms, h_rec, n_rec, h_params, h_voice, voice_stride, &a);
    if (rc != 0) return rc;
    mix_host<short>(a);
    return 0;
}
