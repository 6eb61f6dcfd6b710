// kernels.h -- launch interface between api.cpp (host) and kernels.hip (gfx950 device code).
#pragma once
#include <hip/hip_runtime.h>

namespace gtk {

// workgroup geometry: 11 waves per utterance/stream, time chunks of 16 frames.
// 16 frames x 33 bins = 528 positions = exactly 33 MFMA tiles of 16 positions = 11 waves x 3 tiles,
// so every wave owns the same number of tiles and no MFMA sits behind a branch.
constexpr int TC = 16;
constexpr int NW = 11;
constexpr int NTHR = NW * 64;
constexpr int NT2 = TC * 33 / 16;
constexpr int TPW = NT2 / NW;
// calls of at most SHORT_T frames (streaming steps) run the model kernels with ONE tile per wave: the first 11
// tiles (176 positions) cover every valid position of up to 5 frames, so two thirds of the tile work is skipped
constexpr int SHORT_T = (NW * 16) / 33;           // 5 frames: one tile per wave
constexpr int SHORT_T2 = (2 * NW * 16) / 33;      // 10 frames: two tiles per wave
static_assert(TC * 33 % 16 == 0, "chunk must be a whole number of tiles");
static_assert(NT2 % NW == 0, "tiles must divide evenly over the waves");

// STFT / iSTFT geometry
constexpr int FRAMES_PER_WAVE = 2;   // frames each of the 4 waves of a k_stft workgroup transforms
constexpr int ISTFT_BLOCKS = 7;      // hop blocks one k_istft workgroup emits (from 8 frames: 38 KB of LDS, 4 workgroups per CU)

// per-stream state of hop-level waveform streaming (floats; gtcrn_wave_stream_*): the last 512 input samples (oldest
// first), the windowed second half of the newest frame (the overlap-add tail), an int hop counter (saturating) + pad
constexpr int WS_RING = 0;
constexpr int WS_TAIL = 512;
constexpr int WS_CNT = 768;
constexpr int WS_FLOATS = 772;                   // 3088 B per stream, a multiple of 16
constexpr int WS_CNT_MAX = 1 << 30;
constexpr int WAVE_FRAMES = 2;                   // frames each of the 4 waves of a k_wave_analysis workgroup transforms
static_assert(WS_FLOATS % 4 == 0, "16-byte aligned rows");

// per-stream state (floats).  Rings are indexed by absolute frame number: the conv/TRA rings
// hold 2 rows (row = frame & 1), TCN block k holds 2d rows (row = frame mod 2d, d = 2^k).
constexpr int ST_POS = 0;                        // int frame counter (+3 pad)
constexpr int ST_ENC_H = 4;                      // [3 blocks][2][33][16]
constexpr int ST_ENC_E = ST_ENC_H + 3 * 2 * 33 * 16;   // [3][2][8]
constexpr int ST_G1_H = ST_ENC_E + 48;           // [30 rows][33][16], block k at row 2*(2^k - 1)
constexpr int ST_G2_H = ST_G1_H + 30 * 33 * 16;
constexpr int ST_DEC_H = ST_G2_H + 30 * 33 * 16;
constexpr int ST_DEC_E = ST_DEC_H + 3 * 2 * 33 * 16;
constexpr int ST_FLOATS = ST_DEC_E + 48;         // 38116 floats = 152 464 B per stream

// int8-weight / fp16-activation variant (BASELINE configs[4]); steps > 0 add the tflite path's int8 boundary
struct Quant {
    float in_step = 0.f;    // input quantiser step (calib scale / 255), 0 = fp16 input
    float out_step = 0.f;   // output quantiser step, 0 = fp16 output
};

int configure_kernels();
// lens (optional, device, int32[B]): variable-length batch -- utterance b holds lens[b] <= L samples in its row of
// L, i.e. 1 + lens[b]/256 <= T frames; L and T stay the row strides of every tensor.  nullptr: all rows are full.
int launch_stft(const float* wave, int B, long L, int T, const int* lens, const float* win, const float* twid,
                float* spec, long sb, long sf, long st, float* frames, hipStream_t s);
// 16-bit PCM <-> float32 at the host boundary (n samples, a multiple of 8; dir 0: int16 / 32768, 1: clip(rint(y * 32768)))
int launch_pcm16_convert(const void* src, void* dst, long n, int dir, hipStream_t s);
// G.711 (contract: include/gtcrn_micro_hip.h, "G.711 payloads").  One statement of both laws in integer arithmetic, for
// the host calls (gtcrn_g711_decode_table / gtcrn_g711_encode_pcm16) and the kernels alike: law 0 mu-law, 1 A-law; the
// decoded value and the encoder's input are on the 16-bit linear scale of the PCM16 forms.
constexpr int g711_decode(int law, unsigned c) {
    if (law == 0) {
        const unsigned u = ~c & 0xFFu;
        const int mag = (int)((((u & 15u) << 3) + 132u) << ((u >> 4) & 7u)) - 132;
        return (u & 0x80u) ? -mag : mag;
    }
    const unsigned a = (c ^ 0x55u) & 0xFFu, m = a & 15u, s = (a >> 4) & 7u;
    const int t = s == 0 ? (int)((m << 4) + 8u) : (int)(((m << 4) + 264u) << (s - 1u));
    return (a & 0x80u) ? t : -t;
}
// p in -32768 .. 32767 (the caller clips).  The segment is the position of the leading bit: __builtin_clz.
constexpr unsigned g711_encode(int law, int p) {
    if (law == 0) {
        const int mag = p < 0 ? -p : p;
        const unsigned a = (unsigned)(mag < 32635 ? mag : 32635) + 132u;          // 132 .. 32767
        const unsigned e = 24u - (unsigned)__builtin_clz(a);                      // floor(log2 a) - 7: 0 .. 7
        return ~((p < 0 ? 0x80u : 0u) | (e << 4) | ((a >> (e + 3u)) & 15u)) & 0xFFu;
    }
    const unsigned q = (unsigned)(p >= 0 ? p : ~p) >> 3;                          // 0 .. 4095
    const unsigned s = q < 32u ? 0u : 27u - (unsigned)__builtin_clz(q);           // floor(log2 q) - 4: 1 .. 7
    const unsigned m = (s < 2u ? q >> 1 : q >> s) & 15u;
    return ((p >= 0 ? 0x80u : 0u) | (s << 4) | m) ^ 0x55u;
}
// The one-byte sample types of the packet kernels: the law is a compile-time property of S, as int16 is of `short`.
struct g711u { unsigned char code; static constexpr int law = 0; };
struct g711a { unsigned char code; static constexpr int law = 1; };
static_assert(sizeof(g711u) == 1 && sizeof(g711a) == 1, "a G.711 sample is one byte");
// G.711 codes <-> float32 in bulk (n codes, a multiple of 16; dir 0: D_law[c] / 32768, 1: E_law(clip(rint(y * 32768))))
int launch_g711_convert(const void* src, void* dst, long n, int law, int dir, hipStream_t s);
// gain (optional, device, float[B]): the attenuation limit -- sample n of row b becomes the mix of dry[b * dry_stride + n]
// and the iSTFT's sample with dry gain gain[b] (k_istft_mix); nullptr: the plain kernel
int launch_istft(const float* spec, long sb, long sf, long st, int B, int T, const int* lens, const float* win,
                 const float* twid, float* wave, hipStream_t s, const float* dry = nullptr, long dry_stride = 0,
                 const float* gain = nullptr);
// Which streams a live launch steps.  slots == nullptr: rows 0 .. N-1 of the state range (the IDX = false kernels; cnt is
// not read).  Otherwise (gtcrn_*_slots) row i is the stream whose state sits in slot slots[i] (device, int32[N], in range
// and distinct); cnt (device int32, may be nullptr: N) is clamped to 0..N on the device and rows at or beyond it are neither
// read nor written.  Spectrum / sample rows stay compact (row i of the call), gain is per SLOT, and a launch steps ONE hop /
// frame: a launcher given a table and nhops != 1 returns hipErrorInvalidValue.
struct Rows {
    const int* slots = nullptr;
    const int* cnt = nullptr;
};
// The optional buffers of a live synthesis launch: device memory, per stream or (slot table) per SLOT; nullptr: off
struct WaveOpts {
    const float* gain = nullptr;          // the attenuation limit: one dry gain per stream
    float* meters = nullptr;              // the level-meter records: 4 floats per stream, 16-byte aligned
    float* ramp = nullptr;                // the gain ramps: one float per stream; without `gain` it is not touched
    float* alc = nullptr;                 // the level control: 8 floats per stream, 32-byte aligned, and with them always
    const float* alc_params = nullptr;    // the 16 parameter words
    float* tone = nullptr;                // the tone guard: 8 floats per stream, 32-byte aligned, and with them always
    const float* tone_params = nullptr;   // the 16 parameter words
    const float* tone_table = nullptr;    // gtcrn_tone_table_host's 10 x 256 x 2 floats, 16-byte aligned
};
enum class Synth {      // what k_wave_synthesis does with them: one instantiation per mode and (S, FLUSH, IDX)
    Plain,      // the enhanced block as it is
    // The attenuation limit -- every emitted sample becomes wave_mix(gain[n], dry, sample), in float, before the int16 form's
    // one rounding; the zeros of a first call or an empty flush stay zeros.  Hop h emits block c0 + h - 1: its dry samples
    // are the ring's newest 256 (h == 0: the pairs this lane loads for the ring shift at nhops == 1) or input hop h - 1.
    Mix,
    // The level meters (include/gtcrn_micro_hip.h, "level meters") -- the record meters[4 slot .. 4 slot + 3] = {E_dry,
    // E_out, peak, blocks} is read once, advanced per hop from the emitted floats y and Mix's dry samples x (both 0 for a
    // structural zero block) and stored once by lane 0, before the flush's return.  gain is a run-time branch (null: no mix).
    Meter,
    // Mix / Meter with the gain ramps (include/gtcrn_micro_hip.h, "gain ramps"; gain and ramp both set) -- p = ramp[slot] is
    // the dry gain at which the stream's last emitted block ended.  Both words are the same in every lane (made so for the
    // compiler by a readfirstlane behind hop 0's transform, so `p != g` is a scalar branch and neither load is waited for
    // before the first spectrum is fetched); where they differ, the block of hop 0 mixes sample i with gain_ramp_at(p, g, i)
    // -- this lane's four samples i = 2m, 2m + 1 -- and every other block with g, as Mix does.  A structural zero block
    // stays zeros.  Lane 0 stores g to ramp[slot] behind the hops, in front of the flush's return.
    MixRamp, MeterRamp,
    // The level control (include/gtcrn_micro_hip.h, "level control") -- gain, meters and ramp are run-time branches.  The
    // wave holds the whole block -- this lane's four wet samples w, dry samples x and mixed samples m -- before the first
    // store: E_w, E_x (alc_lane_sum, then wave_sum: the meters' order) and pk = max |m| come first, alc_decide (the host
    // twin's body) advances the record and gives the block's two gains, and y_i = fl(gain_ramp_at(a0, a1, i) m_i) goes to the
    // store and the meters.  The parameter words and the record become scalars behind hop 0's transform, as the ramp words
    // do; lane 0 stores the record (two 16-byte stores) before the flush's return, not after an empty flush.
    Alc,
    // The tone guard (include/gtcrn_micro_hip.h, "tone guard") -- gain, meters, ramp and alc are run-time branches.  Laid out
    // as Alc: the wave holds w and x before the first store.  E_x and the ten P_f come first (tone_lane_dot per table row, then
    // wave_sum_uniform: the butterfly's additions as DPP adds), tone_decide (the host twin's body) advances the record, and a
    // guarded block takes dry gain 1 at every sample; the ramp word p is carried from block to block inside a call.  Level
    // control and the meters then see m as in Alc.  The parameter words and the record become scalars behind hop 0's
    // transform; lane 0 stores the record (two 16-byte stores) before the flush's return, not after an empty flush.  Each lane
    // reads its 4 x 10 table entries per hop from global memory (two 16-byte loads per row, behind the transform).
    Guard
};
constexpr Synth synth_mode(const WaveOpts& o) {      // the ONLY place that turns the pointers into a mode
    return o.tone ? Synth::Guard : o.alc ? Synth::Alc : o.gain && o.ramp ? (o.meters ? Synth::MeterRamp : Synth::MixRamp)
         : o.meters ? Synth::Meter : o.gain ? Synth::Mix : Synth::Plain;
}
// The timing row of a launch (api.cpp): ramps and level control are timed in the row of the form they stand in for.
constexpr Synth synth_timed_as(const WaveOpts& o) { return o.meters ? Synth::Meter : o.gain ? Synth::Mix : Synth::Plain; }
// synth_mode over all 32 null / non-null combinations B; bit 0 of B: gain, 1: meters, 2: ramp, 3: alc with alc_params,
// 4: tone with tone_params and tone_table
template <int... B>
constexpr bool synth_is(Synth want, float x = 0.f) {
    float* const p[2] = {nullptr, &x};
    return ((synth_mode({p[B & 1], p[B >> 1 & 1], p[B >> 2 & 1], p[B >> 3 & 1], p[B >> 3 & 1], p[B >> 4], p[B >> 4], p[B >> 4]}) == want) && ...);
}
static_assert(synth_is<0, 4>(Synth::Plain) && synth_is<1>(Synth::Mix) && synth_is<2, 3, 6>(Synth::Meter));
static_assert(synth_is<5>(Synth::MixRamp) && synth_is<7>(Synth::MeterRamp) && synth_is<8, 9, 10, 11, 12, 13, 14, 15>(Synth::Alc));
static_assert(synth_is<16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31>(Synth::Guard));
// Gain ramps (contract: include/gtcrn_micro_hip.h, "gain ramps"): the dry gain of sample i = 0..255 of a block that ramps
// from p, where the stream's last emitted block ended, to g -- fl(p + fl(fl(g - p) * r_i)), r_i = (i + 1) / 256 (exact), and
// g itself at i == 255 or when p == g.  Three fp32 roundings, never a fused multiply-add (the pragma holds under any
// -ffp-contract of the including file).  One body for the ramped modes of k_wave_synthesis and for gtcrn_gain_ramp_host.
__host__ __device__ inline float gain_ramp_at(float p, float g, int i) {
#pragma clang fp contract(off)
    if (p == g || i == 255) return g;
    const float d = g - p;
    const float s = d * ((float)(i + 1) * 0.00390625f);
    return p + s;
}
// Level control (contract: include/gtcrn_micro_hip.h, "level control"): the block rule, steps 3 .. 9 and 11, once a block's
// three reductions are known.  One body for the Alc mode of k_wave_synthesis and for gtcrn_alc_block_host.  Every
// operation is one correctly rounded fp32 operation (plain operators: the pragma keeps any -ffp-contract of the including
// file from fusing them; `/` and sqrt are the IEEE ones on both sides); the finiteness test reads the bits, so it holds in
// a file compiled with -fno-honor-nans.
struct AlcParams {      // words 0 .. 10 of d_alc_params
    float theta, rho, H, alpha, T, a_min, a_max, d_up, d_dn, c, mode;
};
struct AlcRecord {      // words 0 .. 5 of a stream's record
    float a, S, hang, voice, voiced, blocks;
};
// v >= 0 or NaN: true where v is not <= FLT_MAX
__host__ __device__ inline bool alc_not_finite(float v) {
    return (__builtin_bit_cast(unsigned, v) & 0x7fffffffu) > 0x7f7fffffu;
}
// ((s0^2 + s1^2) + s2^2) + s3^2: a lane's partial sum of a block, the meters' order
__host__ __device__ inline float alc_lane_sum(float s0, float s1, float s2, float s3) {
#pragma clang fp contract(off)
    const float q0 = s0 * s0, q1 = s1 * s1, q2 = s2 * s2, q3 = s3 * s3;
    const float t = q0 + q1;
    const float u = t + q2;
    return u + q3;
}
// Advances the record by one emitted block with energies Ew (wet), Ex (dry) and pk = max |m|; a0 / a1: the gains at which
// the block starts and ends, y_i = fl(gain_ramp_at(a0, a1, i) * m_i).
__host__ __device__ inline void alc_decide(const AlcParams& P, AlcRecord& r, float Ew, float Ex, float pk, float& a0,
                                           float& a1) {
#pragma clang fp contract(off)
    const float a = r.a;
    float at = a, voice = 0.f, lim = a;
    bool limited = false;
    if (!(alc_not_finite(Ew) || alc_not_finite(Ex) || alc_not_finite(pk))) {
        const float rx = P.rho * Ex;
        const bool speech = Ew >= P.theta && Ew >= rx;
        if (speech) {
            r.hang = P.H;
            voice = 1.f;
            if (r.S == 0.f) {
                r.S = Ew;
            } else {
                const float d = Ew - r.S;
                const float s = P.alpha * d;
                r.S = r.S + s;
            }
        } else if (r.hang > 0.f) {
            r.hang = r.hang - 1.f;
            voice = 1.f;
        }
        if (voice != 0.f && r.S > 0.f) {
            const float q = P.T / r.S;
            const float want = fminf(fmaxf(__builtin_sqrtf(q), P.a_min), P.a_max);
            const float lo = a * P.d_dn, hi = a * P.d_up;
            at = fminf(fmaxf(want, lo), hi);
        }
        const float top = pk * fmaxf(a, at);
        if (pk > 0.f && top > P.c) {
            limited = true;
            lim = fmaxf(P.a_min, P.c / pk);
        }
    }
    a0 = limited ? fminf(a, lim) : a;
    a1 = limited ? fminf(at, lim) : at;
    if (P.mode == 0.f) a0 = a1 = 1.f;
    r.a = a1;
    r.voice = voice;
    r.voiced = r.voiced + voice;
    r.blocks = r.blocks + 1.f;
}
// Tone guard (contract: include/gtcrn_micro_hip.h, "tone guard"): the lane product-sum of step 1 and the block rule, steps
// 3 .. 5, once a block's eleven reductions are known.  One body for the Guard mode of k_wave_synthesis and for
// gtcrn_tone_block_host.  Every operation is one correctly rounded fp32 operation; the finiteness test reads the bits.
constexpr int TONE_FREQS = 10;      // 697, 770, 852, 941 (rows), 1209, 1336, 1477, 1633 (columns), 1100, 2100 Hz
struct ToneParams {     // words 0 .. 10 of d_tone_params
    float theta, tau, delta, pi2, pi1, G, N2, N1, H, mode, singles;
};
struct ToneRecord {     // a stream's record
    float tone, cand, run, hold, guard, events, guarded, blocks;
};
// ((x0 t0 + x1 t1) + x2 t2) + x3 t3: a lane's partial sum of a block against one table column (cos or sin of one frequency)
__host__ __device__ inline float tone_lane_dot(float x0, float x1, float x2, float x3, float t0, float t1, float t2, float t3) {
#pragma clang fp contract(off)
    const float p0 = x0 * t0, p1 = x1 * t1, p2 = x2 * t2, p3 = x3 * t3;
    const float t = p0 + p1;
    const float u = t + p2;
    return u + p3;
}
// fl(fl(c^2) + fl(s^2))
__host__ __device__ inline float tone_power(float c, float s) {
#pragma clang fp contract(off)
    const float cc = c * c, ss = s * s;
    return cc + ss;
}
// the first argmax of four values and its value (constant indices only: the array stays in registers)
__host__ __device__ inline int tone_argmax4(const float* P, float& best) {
    int r = 0;
    best = P[0];
#pragma unroll
    for (int j = 1; j < 4; ++j)
        if (P[j] > best) {
            best = P[j];
            r = j;
        }
    return r;
}
// Advances the record by one emitted block with dry energy Ex and powers P[0 .. 9]; r.guard then says whether the block is
// passed dry (when the mode word is 1).  guarded and blocks are step 7's: the caller adds them behind the block.
__host__ __device__ inline void tone_decide(const ToneParams& p, ToneRecord& r, float Ex, const float (&P)[TONE_FREQS]) {
#pragma clang fp contract(off)
    bool finite = !alc_not_finite(Ex);
#pragma unroll
    for (int f = 0; f < TONE_FREQS; ++f) finite = finite && !alc_not_finite(P[f]);
    float cand = 0.f;
    if (finite) {
        float Pr, Pc;
        const int ir = tone_argmax4(P, Pr), ic = tone_argmax4(P + 4, Pc);
        const float er = Pr * 0.0078125f, ec = Pc * 0.0078125f;
        const float tr = p.tau * er, tc = p.tau * ec;
        const float dr = p.delta * Pr, dc = p.delta * Pc;
        bool pair = er >= p.theta && ec >= p.theta && ec <= tr && er <= tc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pair = pair && (j == ir || P[j] <= dr);
            pair = pair && (j == ic || P[4 + j] <= dc);
        }
        const float sum = er + ec;
        const float need = p.pi2 * Ex;
        pair = pair && sum >= need;
        if (pair) {
            cand = (float)(1 + 4 * ir + ic);
        } else if (p.singles != 0.f) {
            const float need1 = p.pi1 * Ex;
            const float e8 = P[8] * 0.0078125f, e9 = P[9] * 0.0078125f;
            if (e8 >= p.theta && e8 >= need1) cand = 17.f;
            else if (e9 >= p.theta && e9 >= need1) cand = 18.f;
        }
    }
    // (values, not stores under branches: the record stays in registers)
    const float run = cand != 0.f ? (cand == r.cand ? r.run + 1.f : 1.f) : 0.f;
    const float need_g = cand < 17.f ? p.G : p.N1, need_r = cand < 17.f ? p.N2 : p.N1;
    const bool hit = cand != 0.f && run >= need_g;
    const bool held = !hit && r.hold > 0.f;
    const float guard = hit || held ? 1.f : 0.f;
    const float hold = hit ? p.H : held ? r.hold - 1.f : r.hold;
    const bool report = cand != 0.f && run >= need_r;
    const float events = report && r.tone != cand ? r.events + 1.f : r.events;
    const float tone = report ? cand : guard == 0.f ? 0.f : r.tone;
    r = ToneRecord{tone, cand, run, hold, guard, events, r.guarded, r.blocks};
}
// hop-level waveform streaming of N streams (gtcrn_wave_stream_step / _flush): S = float or short (int16 PCM).
// analysis: in (N rows of in_stride samples, nhops hops each; flush: r tail samples, nhops = 1) + wstate -> spec, frame-major
// (N, nhops, 257, 2); synthesis (after the model step): spec -> out (N rows of out_stride, 256 nhops samples), advances
// wstate (not on flush).  flush = the end-reflected last frame.  o: the optional buffers; synth_mode(o) picks the kernel.
template <typename S>
int launch_wave_analysis(const S* in, long in_stride, int N, int nhops, int r, bool flush, const float* wstate,
                         const float* win, const float* twid, float* spec, Rows rows, hipStream_t s);
template <typename S>
int launch_wave_synthesis(const float* spec, const S* in, long in_stride, S* out, long out_stride, int N, int nhops, int r,
                          bool flush, float* wstate, const float* win, const float* twid, Rows rows, WaveOpts o, hipStream_t s);
// sample-rate conversion (gtcrn_resample / gtcrn_rate_stream_*): polyphase FIR, taps as a phase table of `up` rows of ntp
// floats (ntp a multiple of 4, rows zero-padded; device memory, 16-byte aligned).  SI / SO = float or short (int16 PCM).
constexpr int RS_THREADS = 256;
constexpr int RS_TILE = 1024;                    // outputs per k_resample workgroup
constexpr int RS_SPAN = 3328;                    // floats of input one tile stages: 48 -> 16 kHz needs 3 * 1023 + 196 + slack
constexpr int RS_LDS_TAPS = 1024;                // phase tables up to this many floats are staged in LDS
constexpr int RATE_SPAN = 1024;                  // per-stream form: history (<= 196) + one hop at the caller's rate (<= 768)
long resample_tile_span(int up, int down, int ntp);
// batch form: row b holds lens[b] (nullptr: L) <= L samples; ceil(len * up / down) outputs per row
template <typename SI, typename SO>
int launch_resample(const SI* in, long in_stride, const int* lens, long L, SO* out, long out_stride, int B, int up, int down,
                    int half, int ntp, const float* taps, hipStream_t s);
// per-stream causal forms (the centred filter delayed by half / down outputs): nhops hops of hin -> 256 (in) or 256 -> hout
// (out) samples per stream; rstate + n * rs_stride = the stream's ntp history floats, read and advanced
template <typename S>
int launch_rate_in(const S* in, long in_stride, float* out, long out_stride, float* rstate, long rs_stride, int N, int nhops,
                   int hin, int up, int down, int ntp, const float* taps, hipStream_t s);
template <typename S>
int launch_rate_out(const float* in, long in_stride, S* out, long out_stride, float* rstate, long rs_stride, int N, int nhops,
                    int hout, int up, int down, int ntp, const float* taps, hipStream_t s);
// high band (gtcrn_rate_stream_step_hb / gtcrn_resample_hb; fs = 24000, 32000, 48000): launch_rate_out with
// fl(wet - fl(g dry[k - 256])) staged instead of the wave step's row (wet, dry: the two 16 kHz hand-offs, one row stride) and
// fl(g in[n - lat]) added at the store, g = hb_gain[stream], lat = H + 2 D; hbstate + n * (256 + lat) = the stream's last 256
// dry samples and last lat input samples as floats, read and advanced.  in and out rows must not overlap.
constexpr int HB_DELAY = 960;                    // the longest delay line: lat at 48 kHz
template <typename S>
int launch_rate_out_hb(const float* wet, const float* dry, long hand_stride, const S* in, long in_stride, S* out, long out_stride,
                       float* rstate, long rs_stride, float* hbstate, const float* hb_gain, int N, int nhops, int hout, int lat,
                       int up, int down, int ntp, const float* taps, hipStream_t s);
// batch form, 16 kHz -> fs: launch_resample of fl(wet - fl(g dry)) (row b: lens[b] <= L samples of each) plus fl(g x[j]) for
// j < xlens[b] <= Lx, g = hb_gain[b]
int launch_resample_hb(const float* wet, long wet_stride, const float* dry, long dry_stride, const int* lens, long L,
                       const float* x, long x_stride, const int* xlens, long Lx, const float* hb_gain, float* out,
                       long out_stride, int B, int up, int down, int half, int ntp, const float* taps, hipStream_t s);
// packet-sized live streaming (gtcrn_packet_stream_*): packets of n samples at the caller's rate = n16 samples at 16 kHz,
// re-blocked on the device to the 256-sample hops of the wave step and back.  Per-stream state row (floats):
// [inbound FIFO PK_FIFO | outbound FIFO PK_FIFO | inbound stage history ntp_in | outbound stage history ntp_out]; both FIFO
// levels are functions of the group's phase (host arithmetic) and are not stored.
constexpr int PK_MAX16 = 4096;                   // longest packet, in 16 kHz samples
constexpr int PK_FIFO = 256;                     // floats of each FIFO between calls (both levels stay below one hop)
constexpr int PK_SEQ = PK_FIFO + PK_MAX16;       // LDS: a FIFO's content ++ what one call appends
constexpr int PK_HIST = 256;                     // LDS in front of the outbound sequence: the outbound stage's history (<= 132)
constexpr int PK_TILE = 256;                     // outputs per staging round of the inbound stage
constexpr int PK_SPAN = 1024;                    // floats of input one round stages: 48 -> 16 kHz needs 3 * 255 + 196 + 1
// The step launchers take their arguments as records, so that no two neighbouring ints can change places unnoticed.
struct PkStage {                                 // a causal resampling stage; ntp == 0: none (16 kHz)
    int up = 1, down = 1, ntp = 0;
    const float* taps = nullptr;
};
struct PkState {                                 // the state rows: ps_stride floats apart, the outbound stage's history
    float* pstate = nullptr;                     // hist_off floats into the row
    long ps_stride = 0;
    int hist_off = 0;
};
struct PkPacket {                                // n samples at the caller's rate = n16 at 16 kHz; g = gcd(n16, 256)
    int n = 0, n16 = 0, g = 0;
};
// Which rows a launch steps and where their hops sit in the hand-off buffer(s).  rows.slots == nullptr: the contiguous form,
// rows 0 .. N-1 at the group's phase phi (the phase BEFORE the call), hop r of row i at hand + i hand_stride + 256 r.
// Otherwise the indexed form of the _slots calls: N = max_active rows named by `rows`, the old phase of row i in phi_rec[i]
// and hop r of it at row pos[r M + i] of round r's block of M rows of 256 floats (what launch_packet_plan wrote).
struct PkRows {
    Rows rows;
    int N = 0;
    int phi = 0;                                 // contiguous
    long hand_stride = 0;
    const int* phi_rec = nullptr;                // indexed
    const int* pos = nullptr;
    int M = 0;
};
// in: N packets (n samples, S) + the inbound FIFOs (phi samples each) -> h = (phi + n16) / 256 hops per stream in `hand`,
// the remainder back in the FIFO.
template <typename S>
int launch_packet_in(const S* in, long in_stride, float* hand, PkPacket pk, PkState st, PkRows rw, PkStage sg, hipStream_t s);
// high band (gtcrn_packet_stream_step_hb / _step_slots_hb; fs = 24000, 32000, 48000; S = float or short): fl(P - fl(gam
// A[t - l16])) staged in the place of the n16 popped samples and fl(gam in[m - lat]) added at the store, gam = gain[stream or
// slot].  hand_a: the inbound hand-off of the same call (rows as `hand`).  hbstate + stream * hb_stride = [the last l16 =
// 512 - g samples of A | the last lat input samples] as floats, read and advanced.  in and out rows must not overlap.
constexpr int PKHB_A = 512;                      // floats of LDS for A's line: l16 <= 511
constexpr int PKHB_DELAY = 1728;                 // the longest input delay line: (511 + 64) * 3 = 1725 samples at 48 kHz
struct PkHighBand {
    const float* hand_a = nullptr;
    float* hbstate = nullptr;
    long hb_stride = 0;
    const float* gain = nullptr;
    int l16 = 0, lat = 0;
};
// out: the outbound FIFOs (lvl = 256 - g - phi samples each) ++ the 256 h samples of the wave step -> n16 popped, resampled
// to n samples (S) per stream, the remainder back in the FIFO.  hb (nullptr: the plain kernels) adds the high band and reads
// the call's input rows `in`.
template <typename S>
int launch_packet_out(const float* hand, const S* in, long in_stride, S* out, long out_stride, PkPacket pk, PkState st,
                      PkRows rw, PkStage sg, const PkHighBand* hb, hipStream_t s);
// packet stream slots (gtcrn_packet_stream_*_slots): the phase is one device word per slot.  plan: for the rows the call
// names (slots / cnt / max_active as in Rows) reads phase[slot], writes per round r < hmax the table tab + r M (the slots
// with more than r hops ready, in row order) and its count cnts[r], per row the record phi_rec[i] (the old phase) and
// pos[r M + i] (the row's place in round r's table, or -1), and advances phase[slot].  M: the row capacity of every array
// and of a round's block of the hand-off buffers (M rows of 256 floats).  The step launchers read the record (PkRows).
int launch_packet_plan(const int* slots, const int* cnt, int max_active, int* phase, int n16, int hmax, int M, int* tab,
                       int* pos, int* phi_rec, int* cnts, hipStream_t s);
// zeroes the packet state rows (ps_stride floats) and the phase words of the listed slots (k_packet_reset_slots)
int launch_packet_reset_slots(float* pstate, long ps_stride, int* phase, const int* slots, const int* cnt, int max_active,
                              hipStream_t s);
// zeroes the high-band rows (hb_stride floats) of the listed slots (k_packet_hb_reset_slots)
int launch_packet_hb_reset_slots(float* hbstate, long hb_stride, const int* slots, const int* cnt, int max_active,
                                 hipStream_t s);
// gspec += adjoint(iSTFT)(gwave): gwave (B, 256 (T-1)) is the gradient w.r.t. the iSTFT output ALREADY divided by
// the window envelope; gspec (B,257,T,2 by strides) receives the gradient w.r.t. the spectrogram (accumulated).
int launch_istft_adjoint(const float* gwave, int B, int T, const float* win, const float* twid, float* gspec, long sb,
                         long sf, long st, hipStream_t s);
int launch_encoder(const float* spec, long sb, long sf, long st, int B, int T, const int* lens, const float* PF,
                   const int* PI, float* en0, float* en1, float* en2, float* en3, float* en4, float* state,
                   unsigned long long* stamps, hipStream_t s, const Quant* q = nullptr, bool front_done = false,
                   const int* pref = nullptr);
// offline front end: STFT (wave) or caller spectrogram -> features, ERB, SFE, en_conv0, en_conv1 (see kernels.hip)
int launch_front(const float* wave, long L, const float* spec_in, long isb, long isf, long ist, int B, int T,
                 const int* lens, const float* win, const float* twid, const float* PF, const int* PI, float* spec_out,
                 float* en0, float* en1p, hipStream_t s, const Quant* q = nullptr);
int launch_gtcn(const float* xin, float* xout, const float* P, int B, int T, float* state, int st_off,
                const float* addend, unsigned long long* stamps, hipStream_t s);
int launch_gtcn_ms(const float* xin, float* xout1, float* xout2, const float* P, int B, float* state, hipStream_t s);
int launch_gtcn_band(const float* xin, float* xout, const float* P, int B, int T, const int* lens, const float* addend,
                     hipStream_t s, const Quant* q = nullptr, const int* pref = nullptr);
int launch_decoder(const float* xg, const float* en0, const float* en1, const float* en2, const float* en3,
                   const float* en4, const float* spec, long sb, long sf, long st, float* out, long osb, long osf,
                   long ost, int B, int T, const int* lens, const float* PF, const int* PI, float* state, float* dbg,
                   unsigned long long* stamps, hipStream_t s, const Quant* q = nullptr, const int* pref = nullptr);
// Variable-length batches in time spans: pref (device, int32[B + 1]) = prefix sums of the utterances' frame counts, made
// from lens by launch_len_prefix (B <= 1024: var_spans_usable); the three per-utterance launchers above then run whole
// rounds of 256 workgroups, each taking an equal share of the frames that exist, instead of one workgroup per utterance.
bool var_spans_usable(int B);
int launch_len_prefix(const int* lens, int B, int T, int* pref, hipStream_t s);
// single-frame streaming step of B streams as ONE launch (encoder -> both GTCN stacks -> decoder, nothing through HBM): four
// streams per workgroup (k_stream_ms), or, wide, stream_wide_streams() of them (k_stream_wide: eight waves x two tiles,
// streamed parameters), the form for stream counts that fill the chip more than once
int launch_stream_step(bool wide, const float* spec, long sb, long sf, float* out, long osb, long osf, int B, const float* PF,
                       const int* PI, float* state, unsigned long long* stamps, Rows rows, hipStream_t s);
// zeroes the model state and (wstate != nullptr) the wave state of the listed slots (k_reset_slots)
int launch_reset_slots(float* state, float* wstate, const int* slots, const int* cnt, int max_active, hipStream_t s);
int stream_wide_streams();
bool stream_ms_usable(long sb, long osb);
int launch_state_convert(float* state, int N, float* conv, float* tra, float* const* tcn8, const int* PI, int dir,
                         hipStream_t s);
int launch_conv2d_causal(const float* x, const float* cache, const float* w, const float* bias, float* y,
                         float* cache_out, int B, int Cin, int Cout, int T, int F, int kt, int kf, int dt, int df,
                         int pf, int groups, int transposed, int Fout, hipStream_t s);
int launch_selftest(const float* A, const float* Bm, const float* C, float* D, hipStream_t s);
// n (a multiple of 4) values -> planes [3][n] and joined [n]; A (16x32), Bm (32x16) -> D (16x16) through split_mm6
int launch_selftest_split3(const float* x, long n, float* planes, float* joined, const float* A, const float* Bm,
                           float* D, hipStream_t s);

}  // namespace gtk
