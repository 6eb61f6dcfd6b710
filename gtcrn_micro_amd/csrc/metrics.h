// metrics.h -- launch interface of metrics.hip: SDR, SI-SNR and STOI of (clean, enhanced) pairs on the device
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
// test hook: n values of a clip's workspace as floats (kind 0 = double, 1 = int)
int launch_score_debug_cvt(const void* src, int kind, float* dst, long n, hipStream_t s);
const char* score_stage_name(int i);

}  // namespace gtm
