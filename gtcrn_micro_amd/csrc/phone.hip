// phone.hip -- telephone-channel rows for resident-corpus batches: the phone plan and the channel kernel (contract:
// include/gtcrn_micro_hip.h, "telephone-channel rows: exact 8 kHz band + G.711").  The arithmetic is
// phone.h's, the very functions phone_host.cpp runs on the host.
//
// One launch over (chunk, row, side).  A workgroup writes CHUNK consecutive outputs of one row of one side (noisy, clean):
//   stage     p over [c0 - 128, c0 - 128 + 2 PPAIRS) as int16 pairs in LDS (step 1; zero outside the row)
//   decimate  thread k of a pass computes v[2n], v[2n + 1] for w pair n (step 2), applies the codec in registers (step 3) and
//             writes the pair; v outside 0 .. J - 1 is zero.  A lane reads the p pairs 2n + m and 2n + 1 + m, m = 0 .. 64: lanes
//             two dwords apart, each pair of reads one aligned 8-byte read, so the wave's reads are conflict-free as ds_read_b64
//   shift     the same w as pairs cut one sample later, so that an output whose window starts on an odd w reads whole pairs too
//   interpolate  a thread writes four consecutive outputs (steps 4 and 5) from 33 + 33 consecutive pairs: lanes one dword apart
// The halo (128 samples of p and 33 pairs of w around the chunk) is recomputed by the neighbouring chunks: 33 / 735 of the
// multiply-adds, which is what buys a single launch with no workspace.  The 32-bit accumulators and why they cannot wrap:
// phone.h, "the accumulators".
#include "phone.h"

namespace gtp {

namespace {

__global__ __launch_bounds__(THREADS) void k_phone_plan(float p, int mask, int B, long item0, const unsigned long long* seed_step,
                                                        PItem* plan) {
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= B) return;
    plan[b] = phone_item(p, mask, item0, seed_step[0], seed_step[1], b);
}

// before the channel: the records with their counters at zero (the channel's workgroups add to them)
__global__ __launch_bounds__(THREADS) void k_phone_records(const PItem* plan, int B, PRecord* rec) {
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= B) return;
    const PRecord r = {codec_in_range(plan[b].codec), 0, 0, 0};
    rec[b] = r;
}

// a chunk of a row, bit for bit: 16 bytes a lane where every row starts on 16 bytes
__device__ inline void copy_chunk(const float* src, float* dst, long c0, long L, bool vec) {
    const long end = c0 + CHUNK < L ? c0 + CHUNK : L;
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    if (vec) {
        for (long i = c0 + 4 * (long)threadIdx.x; i < end; i += 4 * THREADS) {
            if (i + 4 <= end) {
                *reinterpret_cast<uint4*>(d + i) = *reinterpret_cast<const uint4*>(s + i);
            } else {
                for (long k = i; k < end; ++k) d[k] = s[k];
            }
        }
    } else {
        for (long i = c0 + threadIdx.x; i < end; i += THREADS) d[i] = s[i];
    }
}

__global__ __launch_bounds__(THREADS) void k_phone(PhoneArgs a) {
    __shared__ uint32_t s_p[PPAIRS];
    __shared__ uint32_t s_a[VPAIRS];
    __shared__ uint32_t s_b[VPAIRS];
    __shared__ int s_cnt[2 * (THREADS / 64)];
    const int b = blockIdx.x / a.chunks, chunk = blockIdx.x % a.chunks, side = blockIdx.z;
    const long L = a.L, c0 = (long)chunk * CHUNK;
    const float* src = a.src[side] + (long long)b * a.src_stride[side];
    float* dst = a.dst[side] + (long long)b * a.dst_stride[side];
    int codec = codec_in_range(a.plan[b].codec);
    if (codec < 0 || (side == 1 && a.target == 1)) {   // (uniform over the workgroup) a wide-band row, or the wide target
        copy_chunk(src, dst, c0, L, a.vec);
        return;
    }
    if (side == 1) codec = 0;                          // the narrow target: the band without the codec

    // step 1: sample c0 - 128 + 2d and the next one; nothing outside [0, L) is loaded
    for (int d = threadIdx.x; d < PPAIRS; d += THREADS) {
        const long i = c0 - 128 + 2L * d;
        const int lo = i >= 0 && i < L ? pcm_of(src[i]) : 0;
        const int hi = i + 1 >= 0 && i + 1 < L ? pcm_of(src[i + 1]) : 0;
        s_p[d] = pack2(lo, hi);
    }
    __syncthreads();

    // steps 2 and 3: w pair n = c0 / 4 - 16 + k.  Only the pairs of this chunk's own outputs count their clips: the halo's are
    // counted by the chunks that own them.
    const long J = (L + 1) / 2, n0 = c0 / 4 - 16;
    int down = 0, up = 0;
#pragma unroll 1
    for (int k = threadIdx.x; k < VPAIRS; k += THREADS) {
        const long j = 2 * (n0 + k);
        int ca = 0, cb = 0;
        int v0 = decimate_at(s_p + 2 * k, &ca);
        int v1 = decimate_at(s_p + 2 * k + 1, &cb);
        const bool in0 = j >= 0 && j < J, in1 = j + 1 >= 0 && j + 1 < J;      // outside the row there is no v: w is zero
        v0 = in0 ? codec_of(codec, v0) : 0;
        v1 = in1 ? codec_of(codec, v1) : 0;
        s_a[k] = pack2(v0, v1);
        if (k >= 16 && k < 16 + QUADS) down += (in0 ? ca : 0) + (in1 ? cb : 0);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < VPAIRS; k += THREADS) s_b[k] = k ? (s_a[k - 1] >> 16) | (s_a[k] << 16) : 0u;
    __syncthreads();

    // steps 4 and 5
#pragma unroll 1
    for (int t = threadIdx.x; t < QUADS; t += THREADS) {
        const long i = c0 + 4L * t;
        if (i >= L) break;
        int z[4], clip[4];
        interpolate4(s_a + t, s_b + t + 1, z, clip);
        if (a.vec && i + 4 <= L) {
            *reinterpret_cast<float4*>(dst + i) = make_float4(out_of(z[0]), out_of(z[1]), out_of(z[2]), out_of(z[3]));
            up += clip[0] + clip[1] + clip[2] + clip[3];
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (i + q < L) {
                    dst[i + q] = out_of(z[q]);
                    up += clip[q];
                }
        }
    }
    if (side != 0) return;                             // (uniform) the records count the noisy row
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        down += __shfl_xor(down, o, 64);
        up += __shfl_xor(up, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_cnt[threadIdx.x >> 6] = down;
        s_cnt[THREADS / 64 + (threadIdx.x >> 6)] = up;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        int s = 0;
#pragma unroll
        for (int k = 0; k < THREADS / 64; ++k) s += s_cnt[threadIdx.x * (THREADS / 64) + k];
        if (s) atomicAdd(threadIdx.x ? &a.rec[b].saturated_up : &a.rec[b].saturated_down, s);
    }
}

}  // namespace

int launch_phone_plan(float p_phone, int codec_mask, int B, long item0, const unsigned long long* d_seed_step, PItem* d_plan,
                      hipStream_t s) {
    hipLaunchKernelGGL(k_phone_plan, dim3((B + THREADS - 1) / THREADS), dim3(THREADS), 0, s, p_phone, codec_mask, B, item0,
                       d_seed_step, d_plan);
    return (int)hipGetLastError();
}

int launch_phone(PhoneArgs a, hipStream_t s) {
    a.chunks = chunks_of(a.L);
    hipLaunchKernelGGL(k_phone_records, dim3((a.B + THREADS - 1) / THREADS), dim3(THREADS), 0, s, a.plan, a.B, a.rec);
    const dim3 grid((unsigned)((long long)a.B * a.chunks), 1, a.src[1] ? 2 : 1);
    hipLaunchKernelGGL(k_phone, grid, dim3(THREADS), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace gtp
