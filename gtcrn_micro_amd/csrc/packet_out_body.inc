// The body of k_packet_out and k_packet_out_slots (see packet_in_body.inc; GT_PK_IDX false / true).  The including kernel
// provides `srow`, `lvl` and `h` and, indexed, `pos` / `M` (hop r of this row is row pos[r M + row] of round r's block).
    constexpr bool IDX = GT_PK_IDX;
    __shared__ __attribute__((aligned(16))) float s_q[PK_HIST + PK_SEQ];   // [stage history | the FIFO's lvl samples ++ 256 h new]
    __shared__ __attribute__((aligned(16))) float s_t[RS_LDS_TAPS];
    const int tid = threadIdx.x;
    const long row = blockIdx.x;
    float* ps = pstate + srow * ps_stride;
    float* fo = ps + PK_FIFO;
    float* hist = ps + hist_off;
    float* q = s_q + PK_HIST;
    const int whole = 256 * h;
    for (int i = tid; i < lvl; i += RS_THREADS) q[i] = fo[i];
    if constexpr (IDX) {
        for (int i = tid; i < whole; i += RS_THREADS)
            q[lvl + i] = hand[((long)(i >> 8) * M + pos[(long)(i >> 8) * M + row]) * 256 + (i & 255)];
    } else {
        const float* hb = hand + row * hand_stride;
        for (int i = tid; i < whole; i += RS_THREADS) q[lvl + i] = hb[i];
    }
    for (int i = tid; i < ntp; i += RS_THREADS) q[i - ntp] = hist[i];
    const float* tp = ntp ? rs_stage_taps(taps, up * ntp, s_t, tid, RS_THREADS) : nullptr;
    __syncthreads();
    S* o = out + row * out_stride;
    if (ntp == 0) {
        for (int m = tid; m < n; m += RS_THREADS) wave_st<S>(o + m, q[m]);
    } else {
        for (int m = tid; m < n; m += RS_THREADS) {
            const int num = m * down, ih = num / up, k0 = num - ih * up;       // ih < n16
            wave_st<S>(o + m, tp ? rs_dot(tp + k0 * ntp, ntp, q + ih) : rs_dot(taps + (long)k0 * ntp, ntp, q + ih));
        }
        for (int i = tid; i < ntp; i += RS_THREADS) hist[i] = q[n16 - ntp + i];
    }
    const int rem = lvl + whole - n16;                               // < 256: the next call's lvl
    for (int i = tid; i < rem; i += RS_THREADS) fo[i] = q[n16 + i];
