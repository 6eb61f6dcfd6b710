// reverb.hip -- reverberant speech for resident-corpus batches: the reverb plan, the derived tap table, the convolution in
// its plain and its matrix form, and the int8 MFMA self-test (contract: include/gtcrn_micro_hip.h, "reverberant speech:
// exact RIR convolution"); behind them the split convolution, which writes the early or direct target
// beside the wet row in the same pass ("dereverberation targets: early or direct clean").
//
// The convolution is a 64-bit integer sum, so its value does not depend on the order of its terms: both forms, any
// block size and any digit split give the same bits.
//
// Matrix form.  For a 16-group i of outputs, out[16 i + j] = sum_u Hk[j][u] * D[u][i] with Hk[j][u] = h[u + j - 15] (0
// outside the response) and D[u][i] = x[16 i + 15 - u].  Sixteen consecutive u of a column of D are one 16-aligned group
// of sixteen consecutive samples read backwards; both operands are stored with that k order reversed, so a lane's data
// operand is one aligned 16-byte LDS read.  v_mfma_i32_16x16x64_i8 takes Hk as A (row = j) and D as B (column = i):
// lane (i, g) then holds outputs 16 i + 4 g .. + 3 of its tile, four consecutive int16 of the staged row.
// Table of a response (gtcrn_batch_reverb_prepare): group m holds T[m][j][e] = h[16 m + j - e] as two 16 x 16 int8
// tiles, the high digit then the low digit; lane (j, g) of chunk c reads T[4 c + g][j][0 .. 15].
#include "reverb.h"

namespace gtr {

namespace {

using gtb::clampi;
using gtb::Item;

typedef int v4i __attribute__((ext_vector_type(4)));

struct Row {               // row b as the kernels see it; clamped so that no read leaves its clip or its response
    const short* x;
    long long len, s0;
    const short* h;
    int K, rir;            // rir < 0: a dry row (then K = 0)
};

__device__ inline Row row_of(const ReverbArgs& a, int b) {
    const Item it = a.plan[b];
    Row r;
    const int sc = clampi(it.sclip, 0, a.speech.n - 1);
    const long long o0 = a.speech.off[sc], o1 = a.speech.off[sc + 1];
    r.x = a.speech.pcm + o0;
    r.len = o1 > o0 ? o1 - o0 : 0;
    r.s0 = it.sstart > 0 ? it.sstart : 0;
    r.h = nullptr;
    r.K = 0;
    r.rir = a.rplan[b].rir;
    if (r.rir >= 0) {
        if (r.rir > a.n_rir - 1) r.rir = a.n_rir - 1;
        const long long h0 = a.roff[r.rir], h1 = a.roff[r.rir + 1];
        r.K = taps_of(h1 - h0);
        r.h = a.taps + h0;
        if (r.K == 0) r.rir = -1;
    }
    return r;
}

__device__ inline int clip_sample(const Row& r, long long j) { return j >= 0 && j < r.len ? (int)r.x[j] : 0; }

// acc -> the staged sample; returns 1 if it was clamped
__device__ inline int finish(long long acc, short* out) {
    long long v = (acc + 16384) >> 15;
    int sat = 0;
    if (v < -32768) { v = -32768; sat = 1; }
    if (v > 32767) { v = 32767; sat = 1; }
    *out = (short)v;
    return sat;
}

__device__ inline void dry_block(const ReverbArgs& a, const Row& r, short* out, long o0, int block) {
    for (int i = threadIdx.x; i < block; i += THREADS) {
        const long o = o0 + i;
        if (o < a.L) out[o] = (short)clip_sample(r, r.s0 + o);
    }
}

// the workgroup's count of clamped samples -> partial[b][blk]
__device__ inline void put_partial(const ReverbArgs& a, int sat, int* sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sat += __shfl_xor(sat, o, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = sat;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
#pragma unroll
        for (int k = 0; k < THREADS / 64; ++k) s += sm[k];
        a.partial[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(THREADS) void k_reverb_plan(int n_rir, float p, int B, long item0, const unsigned long long* seed_step,
                                                         RItem* rplan) {
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= B) return;
    rplan[b] = reverb_item(n_rir, p, item0, seed_step[0], seed_step[1], b);
}

// ---- the plain form: the contract as it reads, one thread per output sample ------------------------------------------
__global__ __launch_bounds__(THREADS) void k_reverb_plain(ReverbArgs a) {
    __shared__ int sm[THREADS / 64];
    const int b = blockIdx.x / a.blocks, blk = blockIdx.x % a.blocks;
    const Row r = row_of(a, b);
    const long o0 = (long)blk * BLOCK;
    short* out = a.staged + (long long)b * a.stride;
    int sat = 0;
    if (r.rir < 0) {
        dry_block(a, r, out, o0, BLOCK);
    } else {
        for (int i = threadIdx.x; i < BLOCK; i += THREADS) {
            const long o = o0 + i;
            if (o >= a.L) break;
            const long long p = r.s0 + o;             // x[p - k]
            long long acc = 0;
            for (int k = 0; k < r.K; ++k) {
                const long long j = p - k;
                if (j >= 0 && j < r.len) acc += (long long)r.h[k] * (long long)r.x[j];
            }
            sat += finish(acc, out + o);
        }
    }
    put_partial(a, sat, sm);
}

// ---- the matrix form -------------------------------------------------------------------------------------------------
// NT tiles of 256 outputs per wave: a workgroup covers NT * 1024 outputs.  The table's bytes are read once per workgroup
// and chunk (the four waves read the same lines), so the larger block reads a quarter of the smaller one's; the smaller one
// fills the machine from fewer rows (launch_reverb chooses).
template <int NT>
__global__ __launch_bounds__(THREADS, 2) void k_reverb_mfma(ReverbArgs a, bool vec) {
    constexpr int BLK = NT * 256 * (THREADS / 64);
    constexpr int LDS_GROUPS = BLK / 16 + MAX_GROUPS - 1;
    constexpr int DEPTH = 4;                            // chunks of the table in flight per wave
    __shared__ __attribute__((aligned(16))) unsigned char s_hi[LDS_GROUPS * 16];
    __shared__ __attribute__((aligned(16))) unsigned char s_lo[LDS_GROUPS * 16];
    __shared__ int sm[THREADS / 64];
    const int b = blockIdx.x / a.blocks, blk = blockIdx.x % a.blocks;
    Row r = row_of(a, b);
    const long o0 = (long)blk * BLK;
    short* out = a.staged + (long long)b * a.stride;
    const int M = groups_of(r.K);
    const unsigned char* tiles = nullptr;
    long long sumh = 0;
    if (r.rir >= 0) {
        // the response's entry of the table header; an entry that does not lie inside the table (a table of another bank)
        // makes the row dry: wrong audio, no access outside the buffer
        const long long* hd = reinterpret_cast<const long long*>(a.table) + 2 * (long long)r.rir;
        const long long off = hd[0];
        sumh = hd[1];
        if (off < header_bytes(a.n_rir) || (off & 255) || off + (long long)M * GROUP_BYTES > a.table_bytes) r.rir = -1;
        else tiles = a.table + off;
    }
    int sat = 0;
    if (r.rir < 0) {                                   // (uniform over the workgroup)
        dry_block(a, r, out, o0, BLK);
        put_partial(a, 0, sm);
        return;
    }
    // The speech span in LDS, two digit planes.  LDS sample p is window position o0 - 16 (M - 1) + p, p < 16 (BLK / 16 + M - 1).
    const int NG = BLK / 16 + M - 1;
    const long long jbase = r.s0 + o0 - 16LL * (M - 1);
    // eight samples a thread: one 16-byte load (unaligned, as in batch.hip) where the eight lie inside the clip
    for (int p8 = threadIdx.x * 8; p8 < NG * 16; p8 += THREADS * 8) {
        const long long j = jbase + p8;
        short t[8];
        if (j >= 0 && j + 8 <= r.len) {
            __builtin_memcpy(t, r.x + j, sizeof(t));
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) t[q] = (short)clip_sample(r, j + q);
        }
        unsigned hi[2] = {0u, 0u}, lo[2] = {0u, 0u};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int v = t[q];
            hi[q >> 2] |= ((unsigned)(v >> 8) & 255u) << (8 * (q & 3));
            lo[q >> 2] |= (((unsigned)v & 255u) ^ 128u) << (8 * (q & 3));      // (x & 255) - 128 as an int8
        }
        *reinterpret_cast<uint2*>(s_hi + p8) = make_uint2(hi[0], hi[1]);
        *reinterpret_cast<uint2*>(s_lo + p8) = make_uint2(lo[0], lo[1]);
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, g = lane >> 4;
    v4i hh[NT], mid[NT], ll[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        hh[t] = v4i{0, 0, 0, 0};
        mid[t] = v4i{0, 0, 0, 0};
        ll[t] = v4i{0, 0, 0, 0};
    }
    // The table's chunks come in whole fours (groups_of), so the loop body is a fixed sequence of DEPTH chunks x NT tiles with no
    // branch in it.  The tap operands of the DEPTH - 1 chunks ahead are held in registers (a chunk's MFMAs, NT * 64 cycles, do not
    // cover a load from memory) and a tile's data operands are read from LDS while the tile before it multiplies.  A tile behind
    // the row's end is computed like any other and not stored.
    const int C = M / 4;
    const unsigned char* ap = tiles + (size_t)g * GROUP_BYTES + (size_t)li * 16;
    v4i ah[DEPTH], al[DEPTH];
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
        ah[d] = *reinterpret_cast<const v4i*>(ap + (size_t)d * (4 * GROUP_BYTES));
        al[d] = *reinterpret_cast<const v4i*>(ap + (size_t)d * (4 * GROUP_BYTES) + 256);
    }
    // data group of lane (li, g), tile t, chunk c: 16 t + li + (M - 1) - (4 c + g), inside 0 .. NG - 1
    const int q0 = 16 * (wv * NT) + li + M - 1 - g;
    v4i bh = *reinterpret_cast<const v4i*>(s_hi + q0 * 16);
    v4i bl = *reinterpret_cast<const v4i*>(s_lo + q0 * 16);
    for (int c0 = 0; c0 < C; c0 += DEPTH) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            const int c = c0 + d;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int c1 = c + 1 < C ? c + 1 : C - 1;
                const int qn = t + 1 < NT ? q0 + 16 * (t + 1) - 4 * c : q0 - 4 * c1;
                const v4i nh = *reinterpret_cast<const v4i*>(s_hi + qn * 16);
                const v4i nl = *reinterpret_cast<const v4i*>(s_lo + qn * 16);
                hh[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah[d], bh, hh[t], 0, 0, 0);
                mid[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah[d], bl, mid[t], 0, 0, 0);
                mid[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al[d], bh, mid[t], 0, 0, 0);
                ll[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al[d], bl, ll[t], 0, 0, 0);
                bh = nh;
                bl = nl;
                __builtin_amdgcn_sched_barrier(0);     // (keeps the unrolled body from hoisting every LDS read to its top)
            }
            // the slot's next chunk, behind its last reader: the load lands in the registers it frees, DEPTH - 1 chunks ahead
            const int cn = c + DEPTH < C ? c + DEPTH : C - 1;      // (past the end: the last chunk again, not used)
            ah[d] = *reinterpret_cast<const v4i*>(ap + (size_t)cn * (4 * GROUP_BYTES));
            al[d] = *reinterpret_cast<const v4i*>(ap + (size_t)cn * (4 * GROUP_BYTES) + 256);
        }
    }
    const long long bias = 128LL * sumh;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const long o = o0 + 256L * (wv * NT + t) + 16 * li + 4 * g;
        short y[4];
        int s4 = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            s4 += finish(65536LL * hh[t][k] + 256LL * mid[t][k] + (long long)ll[t][k] + bias, y + k) & (int)(o + k < a.L);
        sat += s4;
        if (vec && o + 4 <= a.L) {
            short4 v;
            v.x = y[0]; v.y = y[1]; v.z = y[2]; v.w = y[3];
            *reinterpret_cast<short4*>(out + o) = v;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (o + k < a.L) out[o + k] = y[k];
        }
    }
    put_partial(a, sat, sm);
}

// after the convolution: the records, the staged corpus' offsets table and the rewritten plan
__global__ __launch_bounds__(THREADS) void k_reverb_finish(ReverbArgs a) {
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= a.B) return;
    const Row r = row_of(a, b);
    int sat = 0;
    for (int k = 0; k < a.blocks; ++k) sat += a.partial[(long long)b * a.blocks + k];
    RRecord rec;
    rec.rir = r.rir < 0 ? -1 : r.rir;
    rec.ntaps = r.K;
    rec.saturated = sat;
    rec.reserved = 0;
    a.rec[b] = rec;
    const Item src = a.plan[b];
    const Item it = {b, 0, src.nclip, src.nstart, src.snr_db, src.snr_amp, src.lvl_db, src.lvl_amp};
    a.splan[b] = it;
    a.soffsets[b] = (long long)b * a.stride;
    if (b == a.B - 1) a.soffsets[a.B] = (long long)a.B * a.stride;
}

// ---- the derived table -------------------------------------------------------------------------------------------------
// header: per response {int64 byte offset of its groups, int64 sum of its taps}
__global__ void k_reverb_header(const long long* roff, int n, long long* hd) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    long long off = header_bytes(n);
    for (int r = 0; r < n; ++r) {
        hd[2 * r] = off;
        off += (long long)groups_of(taps_of(roff[r + 1] - roff[r])) * GROUP_BYTES;
    }
    for (long long k = 2LL * n; k < header_bytes(n) / 8; ++k) hd[k] = 0;     // the header's padding: every byte of a table is defined
}

__global__ __launch_bounds__(THREADS) void k_reverb_sum(const short* taps, const long long* roff, long long* hd) {
    __shared__ long long sm[THREADS / 64];
    const int r = blockIdx.x;
    const long long h0 = roff[r];
    const int K = taps_of(roff[r + 1] - h0);
    long long s = 0;
    for (int k = threadIdx.x; k < K; k += THREADS) s += taps[h0 + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) hd[2 * r + 1] = sm[0] + sm[1] + sm[2] + sm[3];
}

// one workgroup per 16-tap group of the whole table
__global__ __launch_bounds__(THREADS) void k_reverb_tiles(const short* taps, const long long* roff, int n, unsigned char* table,
                                                          long long table_bytes) {
    const long long* hd = reinterpret_cast<const long long*>(table);
    const long long pos = header_bytes(n) + (long long)blockIdx.x * GROUP_BYTES;
    if (pos + GROUP_BYTES > table_bytes) return;
    int lo = 0, hi = n - 1;                            // the last response whose groups start at or before pos
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (hd[2 * mid] <= pos) lo = mid; else hi = mid - 1;
    }
    const long long h0 = roff[lo];
    const int K = taps_of(roff[lo + 1] - h0);
    const long long m = (pos - hd[2 * lo]) / GROUP_BYTES;
    if (m >= groups_of(K)) return;                     // (behind the last response)
    const int j = threadIdx.x >> 4, e = threadIdx.x & 15;
    const long long k = 16 * m + j - e;
    const int h = k >= 0 && k < K ? (int)taps[h0 + k] : 0;
    table[pos + threadIdx.x] = (unsigned char)(tap_hi(h) & 255);
    table[pos + 256 + threadIdx.x] = (unsigned char)(tap_lo(h) & 255);
}

// ---- the split convolution: one pass over the speech, two outputs ---------------------------------
// target[i] = the sum over the taps below E, wet[i] = that sum carried on over the rest.  The kernels below are new beside the
// ones above, which they leave as they are.
__device__ inline int split_at(const SplitArgs& a, const Row& r) { return r.rir < 0 ? 0 : split_of(a.split[r.rir], r.K); }

__device__ inline void dry_block2(const ReverbArgs& a, const Row& r, short* wet, short* tgt, long o0, int block) {
    for (int i = threadIdx.x; i < block; i += THREADS) {
        const long o = o0 + i;
        if (o < a.L) {
            const short v = (short)clip_sample(r, r.s0 + o);
            wet[o] = v;
            tgt[o] = v;
        }
    }
}

// the workgroup's two counts of clamped samples -> partial[0][b][blk] (wet), partial[1][b][blk] (target)
__device__ inline void put_partial2(const ReverbArgs& a, int sat, int tsat, int* sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sat += __shfl_xor(sat, o, 64);
        tsat += __shfl_xor(tsat, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        sm[threadIdx.x >> 6] = sat;
        sm[THREADS / 64 + (threadIdx.x >> 6)] = tsat;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        int s = 0;
#pragma unroll
        for (int k = 0; k < THREADS / 64; ++k) s += sm[threadIdx.x * (THREADS / 64) + k];
        a.partial[(long long)threadIdx.x * gridDim.x + blockIdx.x] = s;
    }
}

// the plain form: the contract as it reads, one thread per output sample, two accumulators
__global__ __launch_bounds__(THREADS) void k_split_plain(SplitArgs s) {
    __shared__ int sm[2 * (THREADS / 64)];
    const ReverbArgs& a = s.r;
    const int b = blockIdx.x / a.blocks, blk = blockIdx.x % a.blocks;
    const Row r = row_of(a, b);
    const int E = split_at(s, r);
    const long o0 = (long)blk * BLOCK;
    short* wet = a.staged + (long long)b * a.stride;
    short* tgt = s.target + (long long)b * a.stride;
    int sat = 0, tsat = 0;
    if (r.rir < 0) {
        dry_block2(a, r, wet, tgt, o0, BLOCK);
    } else {
        for (int i = threadIdx.x; i < BLOCK; i += THREADS) {
            const long o = o0 + i;
            if (o >= a.L) break;
            const long long p = r.s0 + o;             // x[p - k]
            long long early = 0;
            for (int k = 0; k < E; ++k) {
                const long long j = p - k;
                if (j >= 0 && j < r.len) early += (long long)r.h[k] * (long long)r.x[j];
            }
            long long acc = early;
            for (int k = E; k < r.K; ++k) {
                const long long j = p - k;
                if (j >= 0 && j < r.len) acc += (long long)r.h[k] * (long long)r.x[j];
            }
            tsat += finish(early, tgt + o);
            sat += finish(acc, wet + o);
        }
    }
    put_partial2(a, sat, tsat, sm);
}

// The response's entry of the split table's header -> the two segments as the matrix form walks them.  E comes from the table
// (the tiles were cut there) and is clamped like any split, so no data index leaves LDS.  False: the segments do not lie inside
// the table (a table of another bank or split); the row then stays dry: wrong audio, no access outside the buffer.
struct Entry {
    const long long* hd;
    const unsigned char* tiles;
    int Ce, Cr, back;                                  // chunks of the two segments; the data side's step back at the seam
};

__device__ inline bool split_entry(const ReverbArgs& a, const Row& r, Entry* en) {
    en->hd = reinterpret_cast<const long long*>(a.table) + 4 * (long long)r.rir;
    const long long off = en->hd[0], e64 = en->hd[3];
    const int E = split_of(e64 < 1 ? 1 : e64 > MAX_TAPS ? MAX_TAPS : (int)e64, r.K);
    const int Me = groups_of(E), Mr = rest_groups(E, r.K);
    en->Ce = Me / 4;
    en->Cr = Mr / 4;
    en->back = en->Ce - rest_first(E) / 4;
    en->tiles = a.table + off;
    return off >= split_header_bytes(a.n_rir) && (off & 255) == 0 && off + (long long)(Me + Mr) * GROUP_BYTES <= a.table_bytes;
}

// The matrix form: k_reverb_mfma's LDS digit planes, register ring of tap chunks, three int32 accumulators per tile and
// epilogue arithmetic, walked over the two segments of the split table.  After the early segment's chunks the accumulators ARE
// the early convolution: the epilogue writes the target row with bias 128 * sum(h[:E]); the accumulators are NOT reset, the rest
// segment's chunks follow and the epilogue writes the wet row with bias 128 * sum(h).  The segments are contiguous, so the ring's
// loads run across the seam; only the data side's chunk index steps back there (the rest segment starts at the 256-tap block
// that holds E).  Zero taps add zero products: every accumulator holds a subset of the terms k_reverb_mfma's holds, and the
// |.| < 2^30 bound of section 7m holds for both epilogues.
template <int NT>
__global__ __launch_bounds__(THREADS, 2) void k_split_mm(SplitArgs s, bool vec) {
    constexpr int BLK = NT * 256 * (THREADS / 64);
    constexpr int LDS_GROUPS = BLK / 16 + MAX_GROUPS - 1;
    constexpr int DEPTH = 4;                            // chunks of the table in flight per wave
    __shared__ __attribute__((aligned(16))) unsigned char s_hi[LDS_GROUPS * 16];
    __shared__ __attribute__((aligned(16))) unsigned char s_lo[LDS_GROUPS * 16];
    __shared__ int sm[2 * (THREADS / 64)];
    const ReverbArgs& a = s.r;
    const int b = blockIdx.x / a.blocks, blk = blockIdx.x % a.blocks;
    Row r = row_of(a, b);
    const long o0 = (long)blk * BLK;
    const int M = groups_of(r.K);
    Entry en;
    if (r.rir >= 0 && !split_entry(a, r, &en)) r.rir = -1;
    if (r.rir < 0) {                                   // (uniform over the workgroup)
        dry_block2(a, r, a.staged + (long long)b * a.stride, s.target + (long long)b * a.stride, o0, BLK);
        put_partial2(a, 0, 0, sm);
        return;
    }
    // The speech span in LDS, two digit planes, as in k_reverb_mfma: LDS sample p is window position o0 - 16 (M - 1) + p.
    const int NG = BLK / 16 + M - 1;
    const long long jbase = r.s0 + o0 - 16LL * (M - 1);
    for (int p8 = threadIdx.x * 8; p8 < NG * 16; p8 += THREADS * 8) {
        const long long j = jbase + p8;
        short t[8];
        if (j >= 0 && j + 8 <= r.len) {
            __builtin_memcpy(t, r.x + j, sizeof(t));
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) t[q] = (short)clip_sample(r, j + q);
        }
        unsigned hi[2] = {0u, 0u}, lo[2] = {0u, 0u};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int v = t[q];
            hi[q >> 2] |= ((unsigned)(v >> 8) & 255u) << (8 * (q & 3));
            lo[q >> 2] |= (((unsigned)v & 255u) ^ 128u) << (8 * (q & 3));      // (x & 255) - 128 as an int8
        }
        *reinterpret_cast<uint2*>(s_hi + p8) = make_uint2(hi[0], hi[1]);
        *reinterpret_cast<uint2*>(s_lo + p8) = make_uint2(lo[0], lo[1]);
    }
    __syncthreads();

    const int Ce = en.Ce, Cr = en.Cr, back = en.back;
    const unsigned char* tiles = en.tiles;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, g = lane >> 4;
    v4i hh[NT], mid[NT], ll[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        hh[t] = v4i{0, 0, 0, 0};
        mid[t] = v4i{0, 0, 0, 0};
        ll[t] = v4i{0, 0, 0, 0};
    }
    // Table chunk c = 0 .. CT - 1 runs through both segments; its data chunk is c in the early segment and c - back in the rest.
    const int CT = Ce + Cr;
    const unsigned char* ap = tiles + (size_t)g * GROUP_BYTES + (size_t)li * 16;
    v4i ah[DEPTH], al[DEPTH];
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
        ah[d] = *reinterpret_cast<const v4i*>(ap + (size_t)d * (4 * GROUP_BYTES));       // (the early segment holds four chunks at least)
        al[d] = *reinterpret_cast<const v4i*>(ap + (size_t)d * (4 * GROUP_BYTES) + 256);
    }
    // data group of lane (li, g), tile t, data chunk c: 16 t + li + (M - 1) - (4 c + g), inside 0 .. NG - 1
    const int q0 = 16 * (wv * NT) + li + M - 1 - g;
    int sat = 0, tsat = 0;
#pragma nounroll
    for (int seg = 0; seg < 2; ++seg) {
        const int cbeg = seg ? Ce : 0, cend = seg ? CT : Ce;
        const int qs = seg ? q0 + 4 * back : q0;       // table chunk c reads data chunk c - back behind the seam
        if (cbeg < cend) {                             // (uniform; the early segment is never empty)
            v4i bh = *reinterpret_cast<const v4i*>(s_hi + (qs - 4 * cbeg) * 16);
            v4i bl = *reinterpret_cast<const v4i*>(s_lo + (qs - 4 * cbeg) * 16);
            for (int c0 = cbeg; c0 < cend; c0 += DEPTH) {
#pragma unroll
                for (int d = 0; d < DEPTH; ++d) {
                    const int c = c0 + d;
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const int c1 = c + 1 < cend ? c + 1 : cend - 1;
                        const int qn = t + 1 < NT ? qs + 16 * (t + 1) - 4 * c : qs - 4 * c1;
                        const v4i nh = *reinterpret_cast<const v4i*>(s_hi + qn * 16);
                        const v4i nl = *reinterpret_cast<const v4i*>(s_lo + qn * 16);
                        hh[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah[d], bh, hh[t], 0, 0, 0);
                        mid[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah[d], bl, mid[t], 0, 0, 0);
                        mid[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al[d], bh, mid[t], 0, 0, 0);
                        ll[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al[d], bl, ll[t], 0, 0, 0);
                        bh = nh;
                        bl = nl;
                        __builtin_amdgcn_sched_barrier(0);     // (keeps the unrolled body from hoisting every LDS read to its top)
                    }
                    // the slot's next chunk, behind its last reader, across the seam: the segments are contiguous
                    const int cn = c + DEPTH < CT ? c + DEPTH : CT - 1;      // (past the end: the last chunk again, not used)
                    ah[d] = *reinterpret_cast<const v4i*>(ap + (size_t)cn * (4 * GROUP_BYTES));
                    al[d] = *reinterpret_cast<const v4i*>(ap + (size_t)cn * (4 * GROUP_BYTES) + 256);
                }
            }
        }
        short* out = (seg ? a.staged : s.target) + (long long)b * a.stride + o0;
        const long long bias = 128LL * en.hd[1 + seg];    // the sum of the taps below E, then of all taps
        // Outputs of this block inside the row.  Opaque per segment: the edge path's per-lane masks would otherwise be hoisted
        // out of this loop and held in scalar registers over the chunk loop, which has none to spare at NT = 8.
        int rem = a.L - o0 < BLK ? (int)(a.L - o0) : BLK;
        asm volatile("" : "+s"(rem));
        int sg = 0;
        if (vec && rem == BLK) {                       // (uniform) the whole block lies inside the row: 8-byte stores, no edge
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                short y[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) sg += finish(65536LL * hh[t][k] + 256LL * mid[t][k] + (long long)ll[t][k] + bias, y + k);
                short4 v;
                v.x = y[0]; v.y = y[1]; v.z = y[2]; v.w = y[3];
                *reinterpret_cast<short4*>(out + 256 * (wv * NT + t) + 16 * li + 4 * g) = v;
            }
        } else {                                       // the row's last block, or rows that do not take 8-byte stores
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int o = 256 * (wv * NT + t) + 16 * li + 4 * g;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    short y;
                    const int c1 = finish(65536LL * hh[t][k] + 256LL * mid[t][k] + (long long)ll[t][k] + bias, &y);
                    if (o + k < rem) {
                        out[o + k] = y;
                        sg += c1;
                    }
                }
            }
        }
        if (seg) sat = sg; else tsat = sg;
    }
    put_partial2(a, sat, tsat, sm);
}

// after the convolution: the 32-byte records, the staged corpora's shared offsets table and the rewritten plan
__global__ __launch_bounds__(THREADS) void k_split_finish(SplitArgs s) {
    const ReverbArgs& a = s.r;
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= a.B) return;
    const Row r = row_of(a, b);
    const long long cells = (long long)a.B * a.blocks;
    int sat = 0, tsat = 0;
    for (int k = 0; k < a.blocks; ++k) {
        sat += a.partial[(long long)b * a.blocks + k];
        tsat += a.partial[cells + (long long)b * a.blocks + k];
    }
    SRecord rec;
    rec.rir = r.rir < 0 ? -1 : r.rir;
    rec.ntaps = r.K;
    rec.saturated = sat;
    rec.split = split_at(s, r);
    rec.target_saturated = tsat;
    rec.r0 = rec.r1 = rec.r2 = 0;
    s.srec[b] = rec;
    const Item src = a.plan[b];
    const Item it = {b, 0, src.nclip, src.nstart, src.snr_db, src.snr_amp, src.lvl_db, src.lvl_amp};
    a.splan[b] = it;
    a.soffsets[b] = (long long)b * a.stride;
    if (b == a.B - 1) a.soffsets[a.B] = (long long)a.B * a.stride;
}

// ---- the split table ---------------------------------------------------------------------------------------------------
__global__ void k_split_header(const long long* roff, const int* split, int n, long long* hd) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    long long off = split_header_bytes(n);
    for (int r = 0; r < n; ++r) {
        const int K = taps_of(roff[r + 1] - roff[r]);
        const int E = K ? split_of(split[r], K) : 0;
        hd[4 * r] = off;
        hd[4 * r + 3] = E;
        if (K) off += (long long)(groups_of(E) + rest_groups(E, K)) * GROUP_BYTES;
    }
    for (long long k = 4LL * n; k < split_header_bytes(n) / 8; ++k) hd[k] = 0;     // the header's padding: every byte of a table is defined
}

__global__ __launch_bounds__(THREADS) void k_split_sum(const short* taps, const long long* roff, long long* hd) {
    __shared__ long long sm[2 * (THREADS / 64)];
    const int r = blockIdx.x;
    const long long h0 = roff[r];
    const int K = taps_of(roff[r + 1] - h0);
    const int E = (int)hd[4 * r + 3];
    long long se = 0, sa = 0;
    for (int k = threadIdx.x; k < K; k += THREADS) {
        const long long h = taps[h0 + k];
        sa += h;
        if (k < E) se += h;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        se += __shfl_xor(se, o, 64);
        sa += __shfl_xor(sa, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        sm[threadIdx.x >> 6] = se;
        sm[THREADS / 64 + (threadIdx.x >> 6)] = sa;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const long long* p = sm + threadIdx.x * (THREADS / 64);
        hd[4 * r + 1 + threadIdx.x] = p[0] + p[1] + p[2] + p[3];
    }
}

// one workgroup per 16-tap group of the whole table
__global__ __launch_bounds__(THREADS) void k_split_tiles(const short* taps, const long long* roff, int n, unsigned char* table,
                                                         long long table_bytes) {
    const long long* hd = reinterpret_cast<const long long*>(table);
    const long long pos = split_header_bytes(n) + (long long)blockIdx.x * GROUP_BYTES;
    if (pos + GROUP_BYTES > table_bytes) return;
    int lo = 0, hi = n - 1;                            // the last response whose groups start at or before pos
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (hd[4 * mid] <= pos) lo = mid; else hi = mid - 1;
    }
    const long long h0 = roff[lo];
    const int K = taps_of(roff[lo + 1] - h0);
    if (K == 0) return;
    const int E = (int)hd[4 * lo + 3];
    const int Me = groups_of(E);
    long long m = (pos - hd[4 * lo]) / GROUP_BYTES;
    if (m >= Me + rest_groups(E, K)) return;           // (behind the last response)
    int k0 = 0, k1 = E;                                // the taps this segment holds
    if (m >= Me) {
        m = m - Me + rest_first(E);
        k0 = E;
        k1 = K;
    }
    const int j = threadIdx.x >> 4, e = threadIdx.x & 15;
    const long long k = 16 * m + j - e;
    const int h = k >= k0 && k < k1 ? (int)taps[h0 + k] : 0;
    table[pos + threadIdx.x] = (unsigned char)(tap_hi(h) & 255);
    table[pos + 256 + threadIdx.x] = (unsigned char)(tap_lo(h) & 255);
}

// ---- the lane maps of v_mfma_i32_16x16x64_i8 -----------------------------------------------------------------------------
// A (16 x 64, row major), B (64 x 16, row major), C and D (16 x 16, row major): lane l holds A[l & 15][16 (l >> 4) + e] and
// B[16 (l >> 4) + e][l & 15] in byte e of its 16-byte operands, and D[4 (l >> 4) + k][l & 15] in register k.
__global__ __launch_bounds__(64) void k_selftest_i8(const signed char* A, const signed char* B, const int* Cm, int* D) {
    const int l = threadIdx.x, li = l & 15, g = l >> 4;
    union { v4i v; signed char c[16]; } fa, fb;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        fa.c[e] = A[li * 64 + 16 * g + e];
        fb.c[e] = B[(16 * g + e) * 16 + li];
    }
    v4i acc;
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = Cm[(4 * g + k) * 16 + li];
    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa.v, fb.v, acc, 0, 0, 0);
#pragma unroll
    for (int k = 0; k < 4; ++k) D[(4 * g + k) * 16 + li] = acc[k];
}

}  // namespace

int launch_reverb_plan(int n_rir, float p_reverb, int B, long item0, const unsigned long long* d_seed_step, RItem* d_rplan,
                       hipStream_t s) {
    hipLaunchKernelGGL(k_reverb_plan, dim3((B + THREADS - 1) / THREADS), dim3(THREADS), 0, s, n_rir, p_reverb, B, item0, d_seed_step,
                       d_rplan);
    return (int)hipGetLastError();
}

int launch_reverb_prepare(const short* d_taps, const long long* d_roff, int n_rir, unsigned char* d_table, long long table_bytes,
                          hipStream_t s) {
    long long* hd = reinterpret_cast<long long*>(d_table);
    hipLaunchKernelGGL(k_reverb_header, dim3(1), dim3(64), 0, s, d_roff, n_rir, hd);
    hipLaunchKernelGGL(k_reverb_sum, dim3(n_rir), dim3(THREADS), 0, s, d_taps, d_roff, hd);
    const long long groups = (table_bytes - header_bytes(n_rir)) / GROUP_BYTES;
    if (groups > 0)
        hipLaunchKernelGGL(k_reverb_tiles, dim3((unsigned)groups), dim3(THREADS), 0, s, d_taps, d_roff, n_rir, d_table, table_bytes);
    return (int)hipGetLastError();
}

int launch_reverb(ReverbArgs a, int form, hipStream_t s) {
    const dim3 block(THREADS);
    const long blk = form == 1 ? BLOCK : block_of(form, a.B, a.L);
    a.blocks = (int)((a.L + blk - 1) / blk);
    const dim3 grid((unsigned)((long long)a.B * a.blocks));
    const bool vec = (reinterpret_cast<uintptr_t>(a.staged) & 7) == 0 && a.stride % 4 == 0;
    if (form == 1) hipLaunchKernelGGL(k_reverb_plain, grid, block, 0, s, a);
    else if (blk == BLOCK) hipLaunchKernelGGL(k_reverb_mfma<BLOCK / 1024>, grid, block, 0, s, a, vec);
    else hipLaunchKernelGGL(k_reverb_mfma<BIG_BLOCK / 1024>, grid, block, 0, s, a, vec);
    hipLaunchKernelGGL(k_reverb_finish, dim3((a.B + THREADS - 1) / THREADS), block, 0, s, a);
    return (int)hipGetLastError();
}

int launch_split_prepare(const short* d_taps, const long long* d_roff, const int* d_split, int n_rir, unsigned char* d_table,
                         long long table_bytes, hipStream_t s) {
    long long* hd = reinterpret_cast<long long*>(d_table);
    hipLaunchKernelGGL(k_split_header, dim3(1), dim3(64), 0, s, d_roff, d_split, n_rir, hd);
    hipLaunchKernelGGL(k_split_sum, dim3(n_rir), dim3(THREADS), 0, s, d_taps, d_roff, hd);
    const long long groups = (table_bytes - split_header_bytes(n_rir)) / GROUP_BYTES;
    if (groups > 0)
        hipLaunchKernelGGL(k_split_tiles, dim3((unsigned)groups), dim3(THREADS), 0, s, d_taps, d_roff, n_rir, d_table, table_bytes);
    return (int)hipGetLastError();
}

int launch_split(SplitArgs a, int form, hipStream_t s) {
    const dim3 block(THREADS);
    const long blk = form == 1 ? BLOCK : block_of(form, a.r.B, a.r.L);
    a.r.blocks = (int)((a.r.L + blk - 1) / blk);
    const dim3 grid((unsigned)((long long)a.r.B * a.r.blocks));
    const bool vec = ((reinterpret_cast<uintptr_t>(a.r.staged) | reinterpret_cast<uintptr_t>(a.target)) & 7) == 0 && a.r.stride % 4 == 0;
    if (form == 1) hipLaunchKernelGGL(k_split_plain, grid, block, 0, s, a);
    else if (blk == BLOCK) hipLaunchKernelGGL(k_split_mm<BLOCK / 1024>, grid, block, 0, s, a, vec);
    else hipLaunchKernelGGL(k_split_mm<BIG_BLOCK / 1024>, grid, block, 0, s, a, vec);
    hipLaunchKernelGGL(k_split_finish, dim3((a.r.B + THREADS - 1) / THREADS), block, 0, s, a);
    return (int)hipGetLastError();
}

int launch_selftest_i8(const signed char* dA, const signed char* dB, const int* dC, int* dD, hipStream_t s) {
    hipLaunchKernelGGL(k_selftest_i8, dim3(1), dim3(64), 0, s, dA, dB, dC, dD);
    return (int)hipGetLastError();
}

}  // namespace gtr
