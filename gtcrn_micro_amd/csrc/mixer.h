// mixer.h -- conference rooms: the mix-minus of the loudest talkers ("conference rooms" in include/gtcrn_micro_hip.h; DESIGN.md
// section 7v).  Steps 1 - 9 of the contract as one set of __host__ __device__ functions (mixer.hip runs them per workgroup on
// the device, mixer_host.cpp per room on the host for gtcrn_mix_rooms_host), the argument record both share and the launch
// interface of mixer.hip.  Both files are compiled with -ffp-contract=off like the batch and phone files: every operation below
// is one correctly rounded fp32 operation, the division included (hipcc's default).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gtm {

constexpr int MAX_ROOM = 1024, MAX_N = 1024, MAX_K = 8, MAX_CONTRIB = 2 * MAX_K, THREADS = 256, LANES = 64;
// Steps 7 and 8 run over spans of SPAN samples, so that the staged blocks of a room (MAX_CONTRIB gained blocks and the common
// sum) fit 64 KB of LDS beside the per-seat arrays whatever n is.
constexpr int SPAN = 512, STAGE_ROWS = MAX_CONTRIB + 1;

struct Seat { int in_row, out_row, rec, reserved; };     // == one seat of d_seats, 16 bytes
struct Record { float g, level, picked, blocks; };        // == one record of d_rec, 16 bytes

struct MixArgs {
    const void* in;            // n_in rows of n samples (float or int16) at in_stride
    void* out;                 // n_out rows at out_stride
    long in_stride, out_stride, voice_stride;
    const int* room_start;     // [R + 1]
    const Seat* seats;         // [n_seats]
    const int* nrooms;         // may be null
    Record* rec;               // [n_rec]
    const float* params;       // [8]
    const float* voice;        // may be null
    int n_in, n_out, n, R, n_seats, n_rec;
    int vec;                   // 1: the output rows take four samples a store (n % 4 == 0, base and stride aligned)
};

struct Params { int K; float theta, alpha, kappa; };
// K of a parameter block that gtcrn_mix_params_host did not make is clamped to 1 .. MAX_K (a NaN counts as 1); theta is step 4's
// fl(theta1 * fl(n)).
__host__ __device__ inline Params params_of(const float* p, int n) {
    const float k = p[0];
    return {k >= 1.0f ? (k <= (float)MAX_K ? (int)k : MAX_K) : 1, p[1] * (float)n, p[2], p[3]};
}

// ---- the tables ---------------------------------------------------------------------------------------------------------------
// The live rooms of a call, and whether room r is run at all.
__host__ __device__ inline int live_rooms(int R, const int* nrooms) {
    if (!nrooms) return R;
    const int k = *nrooms;
    return k < 0 ? 0 : (k < R ? k : R);
}
__host__ __device__ inline bool room_ok(int s0, int s1, int n_seats) {
    return s0 >= 0 && s1 >= s0 && s1 <= n_seats && s1 - s0 <= MAX_ROOM;
}
// A seat as the steps see it: rows outside their range are -1; rec = -1 marks a seat that is ignored altogether.
__host__ __device__ inline Seat seat_of(Seat s, int n_in, int n_out, int n_rec) {
    if (s.rec < 0 || s.rec >= n_rec) return {-1, -1, -1, 0};
    return {s.in_row >= 0 && s.in_row < n_in ? s.in_row : -1, s.out_row >= 0 && s.out_row < n_out ? s.out_row : -1, s.rec, 0};
}

// ---- steps 1 - 5 --------------------------------------------------------------------------------------------------------------
__host__ __device__ inline float sample_of(float v) { return v; }
__host__ __device__ inline float sample_of(short v) { return (float)v * (1.0f / 32768.0f); }   // exact
// Step 1, lane l of 64: the butterfly over the lanes is the caller's (shuffles on the device, a loop on the host).
template <class T>
__host__ __device__ inline float lane_energy(const T* row, int n, int l) {
    float acc = 0.0f;
    for (int j = l; j < n; j += LANES) {
        const float s = sample_of(row[j]);
        acc = acc + s * s;
    }
    return acc;
}
// Step 2: E <= FLT_MAX, read from the bits (a NaN fails it under any compiler flag).
__host__ __device__ inline bool energy_finite(float E) { return (__builtin_bit_cast(uint32_t, E) & 0x7fffffffu) <= 0x7f7fffffu; }

constexpr int F_PRESENT = 1, F_GOLD = 2, F_T = 4, F_CSHIFT = 8;   // flags of a seat; from bit 8 on: its contributor index + 1
struct SeatState { float key, level; int flags; };
// Steps 2 - 5 for a seat of valid rec: `has_in` a valid in_row, E its energy, r its record, `voiced` the voice word != 0 (read
// only when has_voice).
__host__ __device__ inline SeatState seat_state(bool has_in, float E, Record r, bool has_voice, bool voiced, Params p) {
    if (!has_in || !energy_finite(E)) return {-1.0f, r.level, 0};
    const float level = E >= r.level ? E : r.level + p.alpha * (E - r.level);
    const bool gold = r.g == 1.0f;
    const bool eligible = has_voice ? voiced : E >= p.theta;
    return {eligible ? (gold ? p.kappa * level : level) : -1.0f, level, F_PRESENT | (gold ? F_GOLD : 0)};
}
// Step 6's order: a candidate (key a at seat position pa) goes before (b, pb).  Only keys > 0 are candidates.
__host__ __device__ inline bool goes_before(float a, int pa, float b, int pb) { return a > b || (a == b && pa < pb); }
__host__ __device__ inline bool contributes(int flags) { return (flags & F_PRESENT) && (flags & (F_GOLD | F_T)); }

// ---- steps 7 - 9 --------------------------------------------------------------------------------------------------------------
__host__ __device__ inline float fade_gain(int flags, int i, float nf) {
    const float r = (float)(i + 1) / nf;
    return (flags & F_GOLD) ? ((flags & F_T) ? 1.0f : 1.0f - r) : ((flags & F_T) ? r : 0.0f);
}
template <class T>
__host__ __device__ inline float gained(const T* row, int flags, int i, float nf) { return fade_gain(flags, i, nf) * sample_of(row[i]); }
// The stored form of a sum: the float itself, or clip(rint(32768 acc), -32768, 32767), the rule of gtcrn_f32_to_pcm16.
__host__ __device__ inline void put(float* dst, float acc) { *dst = acc; }
__host__ __device__ inline void put(short* dst, float acc) {
    float x = 32768.0f * acc;
    x = x >= -32768.0f ? x : -32768.0f;
    x = x <= 32767.0f ? x : 32767.0f;
    *dst = (short)(int)rintf(x);
}
__host__ __device__ inline Record record_next(Record r, int flags, float level) {
    const float t = (flags & F_T) ? 1.0f : 0.0f;
    return {(flags & F_PRESENT) ? t : 0.0f, (flags & F_PRESENT) ? level : r.level, r.picked + t, r.blocks + 1.0f};
}

// mixer.hip
int launch_mix(const MixArgs& a, int pcm, hipStream_t s);

}  // namespace gtm
