// plc.hip -- packet loss concealment: the row kernel and the reset kernel (contract: include/gtcrn_micro_hip.h, "packet loss
// concealment").  The arithmetic is plc.h's, the very functions plc_host.cpp runs on the host.
//
// One wave per row, four rows per workgroup; the wave branches uniformly on the row's case and nothing crosses waves, so there
// is no workgroup barrier:
//   received, not erased   the row is read once and its n samples go into the ring as int16; nothing else is touched
//   lost                   the history is laid out in logical order in the wave's LDS; when an erasure begins a lane owns a lag
//                          of the coarse grid (two rounds of lanes), the wave reduces over better()'s total order, and the lanes
//                          own the refinement's few lags the same way; then a lane per sample writes the row and the ring
//   received, erased       the last `lag` samples of the history in LDS, a lane per sample of the cross-fade
// No atomics and no scratch: every sample of a row, every ring entry and the record are written by the one lane that owns
// them.  Every index read from a table is checked (slot_of, prm_ok, record_of) before it addresses anything.
#include "plc.h"

namespace gtl {

namespace {

__device__ inline void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The wave's best (score, lag) under better(): six shuffles each way.
__device__ inline void wave_best(double* bs, int* bp) {
#pragma unroll
    for (int d = 1; d < LANES; d <<= 1) {
        const double os = __shfl_xor(*bs, d, LANES);
        const int op = __shfl_xor(*bp, d, LANES);
        if (better(os, op, *bs, *bp)) { *bs = os; *bp = op; }
    }
}

template <class T>
__global__ __launch_bounds__(THREADS) void k_plc(PlcArgs a) {
    __shared__ short s_hist[WAVES][MAX_LH];      // the history in logical order
    __shared__ short s_ana[WAVES][MAX_LH];       // h >> s of the lag search

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int row = blockIdx.x * WAVES + wave;
    if (row >= live_rows(a.M, a.count)) return;
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
        for (int j = keep + lane; j < n; j += LANES) ring[ring_at(r.pos, j, Lh)] = (short)sample_in(x[j], a.law);
        if (lane == 0) a.rec[slot].pos = pos;
        return;
    }

    short* h = s_hist[wave];
    const bool begins = lost && r.erased == 0;
    int P = r.lag;
    for (int j = (begins ? 0 : Lh - P) + lane; j < Lh; j += LANES) h[j] = ring[ring_at(r.pos, j, Lh)];
    wave_sync();

    if (begins) {
        short* an = s_ana[wave];
        int m = 0;
        for (int j = lane; j < Lh; j += LANES) m = max(m, abs16(h[j]));
#pragma unroll
        for (int d = 1; d < LANES; d <<= 1) m = max(m, __shfl_xor(m, d, LANES));
        const int sh = analysis_shift(m);
        for (int j = lane; j < Lh; j += LANES) an[j] = (short)(h[j] >> sh);
        wave_sync();
        double bs = 0.0;
        int bp = NO_LAG;
        for (int p = prm.pmin + lane * prm.D; p <= prm.pmax; p += LANES * prm.D) {
            const double s = score_at(an, Lh, p, prm.D, prm.W);
            if (better(s, p, bs, bp)) { bs = s; bp = p; }
        }
        wave_best(&bs, &bp);
        if (bp == NO_LAG) {
            P = prm.pmax;
        } else {
            const int p0 = bp, lo = refine_lo(p0, prm), hi = refine_hi(p0, prm);
            bs = 0.0;
            bp = NO_LAG;
            for (int p = lo + lane; p <= hi; p += LANES) {
                const double s = score_at(an, Lh, p, 1, prm.W);
                if (better(s, p, bs, bp)) { bs = s; bp = p; }
            }
            wave_best(&bs, &bp);
            P = bp == NO_LAG ? p0 : bp;
        }
    }

    if (lost) {
        for (int j = lane; j < n; j += LANES) {
            const int s = synth(h, Lh, P, j);
            sample_out(x + j, attenuated(s, r.erased + j, prm), a.law);
            if (j >= keep) ring[ring_at(r.pos, j, Lh)] = (short)s;
        }
        if (lane == 0) a.rec[slot] = {pos, P, saturate_erased(r.erased, n, prm), events_next(r.events, begins)};
    } else {
        const int f = prm.F < n ? prm.F : n;
        for (int j = lane; j < n; j += LANES) {
            if (j < f) recover(x + j, attenuated(synth(h, Lh, P, j), r.erased + j, prm), recover_ramp(j, f), a.law);
            if (j >= keep) ring[ring_at(r.pos, j, Lh)] = (short)sample_in(x[j], a.law);
        }
        if (lane == 0) a.rec[slot] = {pos, P, 0, r.events};
    }
}

// A thread per (named slot, history sample); the thread of sample 0 zeroes the record.
__global__ __launch_bounds__(THREADS) void k_plc_reset(short* hist, long hist_stride, Record* rec, int S, const int* params,
                                                       const int* slots, int M, const int* count) {
    const int row = blockIdx.x;
    if (row >= live_rows(M, count)) return;
    const int slot = slot_of(slots, row, S);
    if (slot < 0) return;
    const Prm prm = prm_of(params);
    if (!prm_ok(prm, hist_stride)) return;
    for (int j = threadIdx.x; j < hist_len(prm); j += THREADS) hist[(long)slot * hist_stride + j] = 0;
    if (threadIdx.x == 0) rec[slot] = {0, 0, 0, 0};
}

}  // namespace

int launch_plc(const PlcArgs& a, int kind, hipStream_t s) {
    if (a.M == 0) return 0;
    const dim3 grid((a.M + WAVES - 1) / WAVES), block(THREADS);
    if (kind == 0) hipLaunchKernelGGL(k_plc<float>, grid, block, 0, s, a);
    else if (kind == 1) hipLaunchKernelGGL(k_plc<short>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_plc<code_t>, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

int launch_plc_reset(short* hist, long hist_stride, Record* rec, int S, const int* params, const int* slots, int M,
                     const int* count, hipStream_t s) {
    if (M == 0) return 0;
    hipLaunchKernelGGL(k_plc_reset, dim3(M), dim3(THREADS), 0, s, hist, hist_stride, rec, S, params, slots, M, count);
    return (int)hipGetLastError();
}

}  // namespace gtl
