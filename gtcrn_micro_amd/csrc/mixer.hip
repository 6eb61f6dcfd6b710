// mixer.hip -- conference rooms: the mix kernel (contract: include/gtcrn_micro_hip.h, "conference rooms").
// The arithmetic is mixer.h's, the very functions mixer_host.cpp runs on the host.
//
// One workgroup of four waves per room:
//   energies  a wave per seat (seats wave, wave + 4, ...): step 1's 64 lanes are the wave's, the butterfly six shuffles; lane 0
//             runs steps 2 - 5 and leaves key, level, flags and the output row of the seat in LDS
//   pick      wave 0 runs the K argmax rounds on the keys in LDS (reads only; a lane remembers the picks among its own 16 seat
//             positions in a register mask, so nothing is written between the rounds), then writes the picks and, by ballot
//             and prefix count, the contributors in seat order
//   records   one thread per seat
//   stage     the <= 16 gained contributor blocks of a span of samples, and then their ordered sum, in LDS
//   outputs   one thread per (seat, four samples): the common sum, or for a contributor the ordered sum of the others
// No float atomics and no order that depends on timing: the order of every sum is the contract's.  Every index read from a
// table is checked (seat_of, room_ok) before it addresses anything.
#include "mixer.h"

namespace gtm {

namespace {

template <class T>
__global__ __launch_bounds__(THREADS) void k_mix(MixArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_stage[];     // STAGE_ROWS rows of span samples
    __shared__ float s_key[MAX_ROOM];
    __shared__ float s_level[MAX_ROOM];
    __shared__ int s_flags[MAX_ROOM];
    __shared__ int s_out[MAX_ROOM];
    __shared__ int s_con_in[MAX_CONTRIB];
    __shared__ int s_con_flags[MAX_CONTRIB];
    __shared__ int s_nc;

    const int room = blockIdx.x;
    if (room >= live_rooms(a.R, a.nrooms)) return;
    const int s0 = a.room_start[room], s1 = a.room_start[room + 1];
    if (!room_ok(s0, s1, a.n_seats) || s1 == s0) return;
    const int ns = s1 - s0, n = a.n;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Params prm = params_of(a.params, n);
    const T* in = static_cast<const T*>(a.in);
    T* out = static_cast<T*>(a.out);

    // steps 1 - 5
    for (int p = wave; p < ns; p += THREADS / LANES) {
        const Seat st = seat_of(a.seats[s0 + p], a.n_in, a.n_out, a.n_rec);
        float E = 0.0f;
        if (st.in_row >= 0) {
            E = lane_energy(in + (long)st.in_row * a.in_stride, n, lane);
#pragma unroll
            for (int d = 1; d < LANES; d <<= 1) E = E + __shfl_xor(E, d, LANES);
        }
        if (lane == 0) {
            SeatState ss = {-1.0f, 0.0f, 0};
            if (st.rec >= 0) {
                const bool voiced = a.voice ? a.voice[(long)st.rec * a.voice_stride] != 0.0f : false;
                ss = seat_state(st.in_row >= 0, E, a.rec[st.rec], a.voice != nullptr, voiced, prm);
            }
            s_key[p] = ss.key;
            s_level[p] = ss.level;
            s_flags[p] = ss.flags;
            s_out[p] = st.out_row;
        }
    }
    __syncthreads();

    if (wave == 0) {
        // step 6: bit k of `mine` is the pick of seat position lane + 64 k
        unsigned mine = 0;
        for (int round = 0; round < prm.K; ++round) {
            float bk = -1.0f;
            int bp = MAX_ROOM;
            for (int p = lane, k = 0; p < ns; p += LANES, ++k) {
                const float key = s_key[p];
                if (key > 0.0f && !((mine >> k) & 1u) && goes_before(key, p, bk, bp)) { bk = key; bp = p; }
            }
#pragma unroll
            for (int d = 1; d < LANES; d <<= 1) {
                const float ok = __shfl_xor(bk, d, LANES);
                const int op = __shfl_xor(bp, d, LANES);
                if (goes_before(ok, op, bk, bp)) { bk = ok; bp = op; }
            }
            if (!(bk > 0.0f)) break;                           // (uniform: every lane holds the same winner)
            if ((bp & 63) == lane) mine |= 1u << (bp >> 6);
        }
        // the picks and the contributors, in seat order
        int count = 0;
        for (int base = 0, k = 0; base < ns; base += LANES, ++k) {
            const int p = base + lane;
            int f = 0;
            if (p < ns) f = s_flags[p] | (((mine >> k) & 1u) ? F_T : 0);
            const bool c = contributes(f);
            const unsigned long long votes = __ballot(c);
            const int idx = count + __popcll(votes & ((1ull << lane) - 1ull));
            if (c && idx < MAX_CONTRIB) {
                f |= (idx + 1) << F_CSHIFT;
                s_con_in[idx] = seat_of(a.seats[s0 + p], a.n_in, a.n_out, a.n_rec).in_row;
                s_con_flags[idx] = f;
            }
            if (p < ns) s_flags[p] = f;
            count += __popcll(votes);
        }
        if (lane == 0) s_nc = count < MAX_CONTRIB ? count : MAX_CONTRIB;
    }
    __syncthreads();

    // step 9
    for (int p = tid; p < ns; p += THREADS) {
        const int r = seat_of(a.seats[s0 + p], a.n_in, a.n_out, a.n_rec).rec;
        if (r >= 0) a.rec[r] = record_next(a.rec[r], s_flags[p], s_level[p]);
    }

    // steps 7 and 8, a span of samples at a time
    const int nc = s_nc;
    const float nf = (float)n;
    for (int i0 = 0; i0 < n; i0 += SPAN) {
        const int len = n - i0 < SPAN ? n - i0 : SPAN;
        if (i0) __syncthreads();                           // the last span's readers are done
        for (int c = 0; c < nc; ++c) {
            const T* row = in + (long)s_con_in[c] * a.in_stride;
            const int f = s_con_flags[c];
            for (int i = tid; i < len; i += THREADS) s_stage[c * len + i] = gained(row, f, i0 + i, nf);
        }
        __syncthreads();
        for (int i = tid; i < len; i += THREADS) {
            float acc = 0.0f;
            for (int c = 0; c < nc; ++c) acc = acc + s_stage[c * len + i];
            s_stage[MAX_CONTRIB * len + i] = acc;
        }
        __syncthreads();
        if (a.vec) {
            const int nq = len >> 2;
            for (int u = tid; u < ns * nq; u += THREADS) {
                const int p = u / nq, q = (u - p * nq) << 2;
                const int orow = s_out[p];
                if (orow < 0) continue;
                const int me = (s_flags[p] >> F_CSHIFT) - 1;
                float4 v;
                if (me < 0) {
                    v = *reinterpret_cast<const float4*>(s_stage + MAX_CONTRIB * len + q);
                } else {
                    v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    for (int c = 0; c < nc; ++c) {
                        if (c == me) continue;
                        const float4 w = *reinterpret_cast<const float4*>(s_stage + c * len + q);
                        v.x = v.x + w.x; v.y = v.y + w.y; v.z = v.z + w.z; v.w = v.w + w.w;
                    }
                }
                T* dst = out + (long)orow * a.out_stride + i0 + q;
                alignas(16) T o[4];
                put(o, v.x); put(o + 1, v.y); put(o + 2, v.z); put(o + 3, v.w);
                if (sizeof(T) == 4) *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(o);
                else *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(o);
            }
        } else {
            for (int u = tid; u < ns * len; u += THREADS) {
                const int p = u / len, i = u - p * len;
                const int orow = s_out[p];
                if (orow < 0) continue;
                const int me = (s_flags[p] >> F_CSHIFT) - 1;
                float acc;
                if (me < 0) {
                    acc = s_stage[MAX_CONTRIB * len + i];
                } else {
                    acc = 0.0f;
                    for (int c = 0; c < nc; ++c)
                        if (c != me) acc = acc + s_stage[c * len + i];
                }
                put(out + (long)orow * a.out_stride + i0 + i, acc);
            }
        }
    }
}

}  // namespace

int launch_mix(const MixArgs& a, int pcm, hipStream_t s) {
    if (a.R == 0) return 0;
    const int span = a.n < SPAN ? a.n : SPAN;
    const size_t lds = (size_t)STAGE_ROWS * span * sizeof(float);
    if (pcm) hipLaunchKernelGGL(k_mix<short>, dim3(a.R), dim3(THREADS), lds, s, a);
    else hipLaunchKernelGGL(k_mix<float>, dim3(a.R), dim3(THREADS), lds, s, a);
    return (int)hipGetLastError();
}

}  // namespace gtm
