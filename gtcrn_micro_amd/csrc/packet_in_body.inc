// The body of k_packet_in and k_packet_in_slots (kernels.hip includes this text once into each, with GT_PK_IDX false /
// true): ONE statement of the inbound stage and FIFO arithmetic, and the contiguous kernel stays the plain __global__
// template it was -- same name, same arguments, same instructions.  The including kernel provides `srow` (the stream's row
// of pstate: the call's row, or its slot), `phi` and `h` (the group's, or the row's from the plan record) and, indexed,
// `pos` / `M` (where hop r of this row goes: row pos[r M + row] of round r's block of M rows of 256 floats).
    constexpr bool IDX = GT_PK_IDX;
    __shared__ __attribute__((aligned(16))) float s_a[PK_SEQ];       // the FIFO's phi samples ++ this packet at 16 kHz
    __shared__ __attribute__((aligned(16))) float s_x[PK_SPAN];
    __shared__ __attribute__((aligned(16))) float s_t[RS_LDS_TAPS];
    const int tid = threadIdx.x;
    const long row = blockIdx.x;
    const S* x = in + row * in_stride;
    float* ps = pstate + srow * ps_stride;
    for (int i = tid; i < phi; i += RS_THREADS) s_a[i] = ps[i];
    if (ntp == 0) {                                                  // 16 kHz: the packet as it is
        for (int m = tid; m < n16; m += RS_THREADS) s_a[phi + m] = wave_ld<S>(x + m);
        __syncthreads();
    } else {
        float* hist = ps + 2 * PK_FIFO;
        const float* tp = rs_stage_taps(taps, up * ntp, s_t, tid, RS_THREADS);
        for (int m0 = 0; m0 < n16; m0 += PK_TILE) {
            const int m1 = m0 + PK_TILE < n16 ? m0 + PK_TILE : n16;
            const int lo = (m0 * down) / up - (ntp - 1), cnt = ((m1 - 1) * down) / up - lo + 1;   // <= PK_SPAN (launch check)
            for (int i = tid; i < cnt; i += RS_THREADS) {
                const int g = lo + i;                                // >= 1 - ntp; < n
                s_x[i] = g >= 0 ? wave_ld<S>(x + g) : hist[ntp + g];
            }
            __syncthreads();
            for (int m = m0 + tid; m < m1; m += RS_THREADS) {
                const int num = m * down, ih = num / up, k0 = num - ih * up;
                const float* xs = s_x + (ih - lo);
                s_a[phi + m] = tp ? rs_dot(tp + k0 * ntp, ntp, xs) : rs_dot(taps + (long)k0 * ntp, ntp, xs);
            }
            __syncthreads();
        }
        for (int i = tid; i < ntp; i += RS_THREADS) hist[i] = wave_ld<S>(x + n - ntp + i);        // (ntp <= n)
    }
    const int whole = 256 * h, rem = phi + n16 - whole;              // rem < 256: the next call's phi
    if constexpr (IDX) {
        // (RS_THREADS == 256: a thread's hop index i >> 8 is workgroup uniform in every pass)
        for (int i = tid; i < whole; i += RS_THREADS)
            hand[((long)(i >> 8) * M + pos[(long)(i >> 8) * M + row]) * 256 + (i & 255)] = s_a[i];
    } else {
        float* o = hand + row * hand_stride;
        for (int i = tid; i < whole; i += RS_THREADS) o[i] = s_a[i];
    }
    for (int i = tid; i < rem; i += RS_THREADS) ps[i] = s_a[whole + i];
