// metrics.h -- launch interface of metrics.hip: SDR, SI-SNR, STOI, ESTOI and segmental SNR of (clean, enhanced) pairs on the device
// ("scores" in include/gtcrn_micro_hip.h).  metrics_host.cpp designs the tables and checks the arguments.
#pragma once
#include <hip/hip_runtime.h>

namespace gtm {

constexpr int SC_UP = 5, SC_DOWN = 8, SC_HALF = 256, SC_NTAPS = 2 * SC_HALF + 1;   // the 16 kHz -> 10 kHz stage
constexpr int SC_FRAME = 256, SC_HOP = 128, SC_NFFT = 512, SC_BANDS = 15, SC_SEG = 30;
constexpr int SC_STAGES = 6;           // launches of one gtcrn_score with STOI asked for

struct ScoreRecord {                   // == gtcrn_score_record
    double sdr, sisnr, stoi;
    int kept_frames, segments;
};

// header words a clip's workspace begins with (ints)
enum { SC_H_LEN = 0, SC_H_N10, SC_H_NFR, SC_H_K, SC_H_M, SC_H_WORDS = 16 };

// A clip's workspace, every offset in bytes from the clip's base and a multiple of 16; a function of L alone.
struct ScoreLayout {
    long n10 = 0, nfr = 0;             // 10 kHz samples and analysis frames of an L-sample clip
    long x10_stride = 0;               // floats between the 10 kHz ref and inf signals
    long env_stride = 0;               // floats between two bands of an envelope; 15 of them between ref and inf
    long o_x10 = 0, o_edb = 0, o_kept = 0, o_flag = 0, o_env = 0;
    long clip_bytes = 0;
};

__host__ __device__ inline long score_n10(long len) { return (len * SC_UP + SC_DOWN - 1) / SC_DOWN; }
// frame starts 0, 128, ... < n10 - 256 (strict)
__host__ __device__ inline long score_frames_of(long n10) { return n10 > SC_FRAME ? (n10 - SC_FRAME + SC_HOP - 1) / SC_HOP : 0; }
ScoreLayout score_layout(long L);

struct ScoreTables {                   // device pointers, designed in double by metrics_host.cpp
    const float* taps = nullptr;       // 513 taps, sum 5
    const double* win = nullptr;       // 256-point window, and the same rounded to float
    const float* winf = nullptr;
    const float2* tw256 = nullptr;     // exp(-2 pi i k / 256), k < 256
    const float2* tw512 = nullptr;     // exp(-2 pi i k / 512), k < 256
    const int* bands = nullptr;        // lo[15] then hi[15]
};

struct ScorePlan {
    const float* ref = nullptr;
    const float* inf = nullptr;
    long ref_stride = 0, inf_stride = 0;
    const int* lens = nullptr;
    long L = 0;
    int B = 0, what = 0;
    ScoreRecord* out = nullptr;
    char* ws = nullptr;
    ScoreLayout lay;
    ScoreTables tab;
};

// The launches of one call, in stream order.  ev (optional): SC_STAGES + 1 events recorded around them.
int launch_score(const ScorePlan& p, hipStream_t s, hipEvent_t* ev);

// ---- gtcrn_score_ext: the same launches, then ESTOI, segmental SNR and the 64-byte record
constexpr int SX_STAGES = SC_STAGES + 3;                       // launches of one gtcrn_score_ext with everything asked for
constexpr int SX_FRAME = 480, SX_HOP = 120;                    // segmental SNR: 30 ms frames every 7.5 ms at 16 kHz
constexpr int SX_SEGS_PER_WG = 8;                              // ESTOI segments per workgroup (two per wave)
constexpr int SX_RUN = 32;                                     // segmental-SNR frames per workgroup

struct ScoreExtRecord {                // == gtcrn_score_ext_record
    ScoreRecord base;
    double estoi, segsnr;
    int segsnr_frames, zero[3];
};

__host__ __device__ inline long score_segsnr_frames_of(long n) { return n >= SX_FRAME ? (n - SX_FRAME) / SX_HOP + 1 : 0; }

// The ext workspace: B 32-byte records (what the six kernels above write), then B clip slices of clip_bytes each; a slice
// is the ScoreLayout slice followed by the clip's d_s (o_ds) and per-frame v (o_v), both double.
struct ScoreExtPlan {
    ScorePlan base;                    // out = the records at the head of the workspace, ws behind them, what & 7,
                                       // lay.clip_bytes = the ext slice
    int what = 0;                      // all five bits
    long o_ds = 0, o_v = 0;
    long max_segments = 0, max_frames = 0;   // S and F of an L-sample clip
    const double* w480 = nullptr;      // the segmental-SNR window (device)
    ScoreExtRecord* out = nullptr;
};
ScoreExtPlan score_ext_layout(long L);     // base.lay, o_ds, o_v, max_segments, max_frames; the rest left empty
inline size_t score_ext_bytes(int B, long L) { return (size_t)B * (sizeof(ScoreRecord) + (size_t)score_ext_layout(L).base.lay.clip_bytes); }
// ev (optional): SX_STAGES + 1 events
int launch_score_ext(const ScoreExtPlan& p, hipStream_t s, hipEvent_t* ev);
const char* score_ext_stage_name(int i);
// test hook: n values of a clip's workspace as floats (kind 0 = double, 1 = int)
int launch_score_debug_cvt(const void* src, int kind, float* dst, long n, hipStream_t s);
const char* score_stage_name(int i);

}  // namespace gtm
