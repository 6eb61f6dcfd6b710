// The body of k_packet_out_hb and k_packet_out_slots_hb (GT_PK_IDX false / true): packet_out_body.inc with the high band
// carried around the model.  The including kernel provides `srow`, `phi` (the phase BEFORE this call's inbound stage), `lvl`
// and `h` and, indexed, `pos` / `M`.  With gam = hb_gain[srow], A the stream's inbound 16 kHz sequence and P what the outbound
// FIFO pops (both counted from the stream's reset), l16 = 512 - g and lat the form's latency at fs:
//     s[t] = fl(P[t] - fl(gam A[t - l16]))   staged in the place of the n16 popped samples (the remainder that returns to the
//                                            FIFO stays raw P; the outbound history then holds s)
//     out[m] = fl(stage(s)[m] + fl(gam x[m - lat]))
// State row (floats, hb_stride apart): [the last l16 samples of A | the last lat input samples], zeros after a reset.
// This call's n16 new samples of A are where k_packet_in left them: index phi + k of "old inbound FIFO ++ packet" lies in hop
// (phi + k) >> 8 of the inbound hand-off while below 256 h, else in the inbound FIFO of the packet state (neither is written
// here; the wave step writes the other hand-off).  Every word of the state rows is read into LDS before the barrier and
// written after it by the thread that owns its index: with n < lat most of the delay line survives a call and moves.
    constexpr bool IDX = GT_PK_IDX;
    __shared__ __attribute__((aligned(16))) float s_q[PK_HIST + PK_SEQ];   // [stage history | the FIFO's lvl samples ++ 256 h new]
    __shared__ __attribute__((aligned(16))) float s_t[RS_LDS_TAPS];
    __shared__ float s_sa[PKHB_A];                                    // the last l16 samples of A
    __shared__ float s_dl[PKHB_DELAY];                                // the last lat input samples
    const int tid = threadIdx.x;
    const long row = blockIdx.x;
    const float gam = hb_gain[srow];
    float* ps = pstate + srow * ps_stride;
    float* fo = ps + PK_FIFO;
    float* hist = ps + hist_off;
    float* sa = hbstate + srow * hb_stride;
    float* dl = sa + l16;
    const S* x = in + row * in_stride;
    float* q = s_q + PK_HIST;
    const int whole = 256 * h;
    // new sample k < n16 of A (this call's)
    const auto new_a = [&](int k) -> float {
        const int i = phi + k;
        if (i >= whole) return ps[i - whole];
        if constexpr (IDX) return hand_a[((long)(i >> 8) * M + pos[(long)(i >> 8) * M + row]) * 256 + (i & 255)];
        else return hand_a[row * hand_stride + i];
    };
    // A[t - l16] for popped sample m of this call: the state's, then this call's own
    const auto old_a = [&](int m) -> float { return m < l16 ? sa[m] : new_a(m - l16); };
    for (int i = tid; i < lvl; i += RS_THREADS) {
        const float p = fo[i];
        q[i] = i < n16 ? __fsub_rn(p, __fmul_rn(gam, old_a(i))) : p;
    }
    for (int i = tid; i < whole; i += RS_THREADS) {
        float p;
        if constexpr (IDX) p = hand[((long)(i >> 8) * M + pos[(long)(i >> 8) * M + row]) * 256 + (i & 255)];
        else p = hand[row * hand_stride + i];
        const int m = lvl + i;
        q[m] = m < n16 ? __fsub_rn(p, __fmul_rn(gam, old_a(m))) : p;
    }
    for (int i = tid; i < ntp; i += RS_THREADS) q[i - ntp] = hist[i];
    for (int i = tid; i < l16; i += RS_THREADS) s_sa[i] = sa[i];
    for (int i = tid; i < lat; i += RS_THREADS) s_dl[i] = dl[i];
    const float* tp = rs_stage_taps(taps, up * ntp, s_t, tid, RS_THREADS);      // (never nullptr: the launchers check)
    __syncthreads();
    S* o = out + row * out_stride;
    for (int m = tid; m < n; m += RS_THREADS) {
        const int num = m * down, ih = num / up, k0 = num - ih * up;           // ih < n16
        const float xd = m >= lat ? wave_ld<S>(x + (m - lat)) : s_dl[m];
        wave_st<S>(o + m, __fadd_rn(rs_dot(tp + k0 * ntp, ntp, q + ih), __fmul_rn(gam, xd)));
    }
    for (int i = tid; i < ntp; i += RS_THREADS) hist[i] = q[n16 - ntp + i];
    const int rem = lvl + whole - n16;                               // < 256: the next call's lvl
    for (int i = tid; i < rem; i += RS_THREADS) fo[i] = q[n16 + i];
    // both delay lines advance: the last l16 of (A's line ++ n16 new), the last lat of (x's line ++ the packet)
    for (int i = tid; i < l16; i += RS_THREADS) sa[i] = n16 + i < l16 ? s_sa[n16 + i] : new_a(n16 + i - l16);
    for (int i = tid; i < lat; i += RS_THREADS) dl[i] = n + i < lat ? s_dl[n + i] : wave_ld<S>(x + (n + i - lat));
