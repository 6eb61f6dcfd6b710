// The body of k_stream_ms and k_stream_ms_slots (kernels.hip includes this text once into each, with GT_SM_IDX false /
// true): ONE source for the contiguous and the indexed single-launch step, and the contiguous kernel stays the plain
// __global__ function it was -- same name, same arguments, same instructions.  See the comments in front of k_stream_ms.
    constexpr bool IDX = GT_SM_IDX;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if constexpr (IDX) {
        NB = slot_count(cnt, NB);
        if (NB - (int)blockIdx.x * SmLds::NS <= 0) {              // (workgroup uniform; nothing issued, no barrier met)
            STAMP_ZERO(stamps)
            return;
        }
    }
    stagger_start(stagger);
    STAMP_INIT(SS)
    using LD = SmLds;
    constexpr int RW = LD::RW, NS = LD::NS;
    constexpr bool SPLIT = kSplitDense;
    float* sPE = smem + LD::PE;
    float* sPG = smem + LD::PG;
    float* sPD = smem + LD::PD;
    int* sI = reinterpret_cast<int*>(smem + LD::I);
    float* sBS = smem + LD::BS;
    float* sEHe = smem + LD::EHE;
    float* sEHd = smem + LD::EHD;
    int* sTB = reinterpret_cast<int*>(smem + LD::TB);
    float* sG = smem + LD::G;
    float* sEN0 = smem + LD::EN0;
    const Lane L = lane_info();
    const int tid = L.tid, n = L.n, g = L.g;
    const int b = blockIdx.x;
#ifdef GT_EXP_SAMESTATE   // timing experiment only (results are wrong): every workgroup works on the state of one of eight -- all
    float* stb = state + (long)(b & 7) * NS * ST_FLOATS;       // state traffic hits in L2: what the step costs without HBM latency
#else
    float* stb = state + (IDX ? 0L : (long)b * NS * ST_FLOATS);   // first stream of this workgroup (IDX: slot 0, see SROW)
#endif
    const int nlive = min(NS, NB - b * NS), nfr = nlive;
    [[maybe_unused]] volatile int* sSlot = reinterpret_cast<int*>(smem + LD::FLOATS);   // IDX: the slot ids (see SROW)
    if constexpr (IDX) {
        static_assert(NS <= SLOT_WORDS && (LD::FLOATS + SLOT_WORDS) * 4 <= 160 * 1024, "slot words behind the images");
        if (tid < SLOT_WORDS) sSlot[tid] = slots[b * NS + min(tid, nlive - 1)];
        wg_barrier();
    }
    const Tiles<1> tt = make_tiles<1>(L);
    const int row = min(tt.tl[0], NS - 1);                      // the lane's stream (tail lanes of the tile geometry: clamped)
    const bool lane_live = tt.tl[0] < nlive;
    [[maybe_unused]] float* stl = stb + SROW(lane_live ? tt.tl[0] : 0);   // ... its state
    // (IDX: formed anew from the slot word at every use -- a 64-bit pointer per lane held through the step does not fit)
#define STL(i) (IDX ? stb + SROW(lane_live ? tt.tl[0] : 0) : stl)

    // the dense 3x3 of decoder block j -> stage buffer by LDS-DMA (see k_decoder)
    constexpr int DN_PIECES = (SPLIT ? DN16_SIZE : 9 * 256) / 256;
    auto dense_fetch = [&](int j) {
        const float* src = PF + P_DEC + (SPLIT ? D_DN16 + j * DN16_SIZE : D_BLK + j * GBD_SIZE + GB_DN_A);
        int lz = L.lane;
        asm volatile("" : "+v"(lz));
        for (int pi = L.wave; pi < DN_PIECES; pi += NW) {
            const float* gsrc = src + pi * 256 + 4 * lz;
            const unsigned lds_dst = (unsigned)(size_t)(__attribute__((address_space(3))) void*)(sPD + DL_DN + pi * 256);
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep)
                         : "v"(gsrc), "s"(lds_dst)
                         : "memory");
        }
    };
    // history rows of one block, all streams of the workgroup: [NS][2 rows (frame parity)][33][16] of the state ->
    // two 16-byte items per thread; written to the block's LDS image later (pad columns are zeroed once per phase)
    auto hist_fetch = [&](int st_off, f32x4 (&v)[2]) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int i = tid + q * NTHR, sidx = i / 264, r = i - sidx * 264;
            const bool ok = i < NS * 264 && sidx < nlive;
            v[q] = ld4(stb + (ok ? SROW(sidx) + st_off + r * 4 : SROW(0) + ST_ENC_H));   // clamped: a valid record
        }
    };
    auto hist_store = [&](float* img, auto split, const f32x4 (&v)[2]) {
        constexpr bool SP = decltype(split)::value;
        constexpr int RS = SP ? RS_WIDE : 16;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int i = tid + q * NTHR, sidx = i / 264, r = i - sidx * 264;
            if (i < NS * 264) {
                const int rw = r >= 132 ? 1 : 0, rr = r - rw * 132;
                const f32x4 val = sidx < nlive ? v[q] : splat(0.f);
                const int rec = (sidx * 2 * 35 + rw * 35 + 1 + (rr >> 2)) * RS;
                if constexpr (SP) st_split(img, rec, rr & 3, val);
                else st4(img + rec + 4 * (rr & 3), val);
            }
        }
    };
    auto hist_zero_pads = [&](float* img, int rs) {               // columns 0 and 34 of the NS * 2 image rows
        if (tid < NS * 2 * 2 * 8) {
            const int rw = tid >> 4, side = (tid >> 3) & 1, gg = tid & 7;
            if (gg < rs / 4) st4(img + (rw * 35 + side * 34) * rs + 4 * gg, splat(0.f));
        }
    };

    // ------------------------------------------------------------------------------------------------- prologue
    // Every parameter segment is resident in LDS for the whole step (86 KB); they arrive by LDS-DMA in the order of their
    // first use, and only what the front end needs is waited for at the first barrier:
    //   group A  encoder front end (ERB bands, SFE, en_convs.0/1: 9 KB)          -> waited for here (one piece per wave)
    //   group B  the three encoder blocks                                         -> counted wait at the barrier behind en_conv1
    //   group C  both GTCN stacks;  group D  decoder blocks, de_convs.3/4, ERB.bs table, block 0's dense planes
    // B, C, D (7 pieces per wave) are issued BEHIND the consumption of this phase's register loads (spectrogram, first
    // history rows, integer tables) and are in flight during the front end's four phases.
    static_assert(P_GTCN == P_ENC + ENC_SIZE && (ENC_SIZE + 2 * GTCN_SIZE) % 4 == 0, "encoder + GTCN segments are contiguous");
    constexpr bool SPLIT3 = SPLIT && kSplitDe3;
    {
        const DmaSeg ga[1] = {{P_ENC, LD::PE, E_BLK}};
        static_assert((E_BLK + 255) / 256 <= NW, "group A: one piece per wave");
        lds_dma_group<1, 1, NW>(ga, PF, smem, L.wave, L.lane);
    }
    for (int i = tid; i < P_INTS - ENC_I_SKIP; i += NTHR) sI[i] = PI[i < I_BS_LO ? i : i + ENC_I_SKIP];
    if (tid < NS * 48) {
        const int sidx = tid / 48, e = tid - sidx * 48;
        sEHe[tid] = sidx < nlive ? stb[SROW(sidx) + ST_ENC_E + e] : 0.f;
        sEHd[tid] = sidx < nlive ? stb[SROW(sidx) + ST_DEC_E + e] : 0.f;
    }
    if (tid < 8) sTB[tid] = tid < nlive ? reinterpret_cast<const int*>(stb + SROW(tid))[0] : 0;
    f32x4 hv[2];
    hist_fetch(ST_ENC_H, hv);
    hist_zero_pads(smem + LD::HE, 16);

    // ------------------------------------------------------------------------------------------------- encoder
    // (the front end and the three depthwise GTConv blocks of k_encoder<1, true, false, true>: same expressions)
    float* sSpec = smem + LD::A;
    float* sE0 = smem + LD::A;
    float* sWe = smem + LD::A;
    float* sSe = smem + LD::SE;
    float* sEB = smem + LD::B;
    float* sF0 = sEB + 3 * RW * EB_ROW;
    // rows = streams.  Items always run bin-fastest here: the frame-fastest decomposition of spec_item_first assumes
    // 16-row chunks, and a stream stride below the bin stride is not a layout worth a second path.
    constexpr bool t_fast = false;
    const int sf32 = (int)sf, st32 = (int)sb;
    constexpr int SPEC_ITEMS = (RW * NBINS + NTHR - 1) / NTHR;
    float2 spn[SPEC_ITEMS];                                        // kept for the mask at the end of the step
    {
        const float* base = spec + (long)b * NS * sb;
        int tl, f;
        spec_item_first(tid, t_fast, tl, f);
#pragma unroll
        for (int q = 0; q < SPEC_ITEMS; ++q) {
            const bool ok = tl < nfr && f < NBINS;
            spn[q] = *reinterpret_cast<const float2*>(base + (ok ? f * sf32 + tl * st32 : 0));
            spec_item_next(t_fast, tl, f);
        }
    }
    hist_store(smem + LD::HE, std::false_type{}, hv);
    if (tid < 3 * RW * 9) {                                        // zero pad entries of EB / F0
        const int rw = tid / 9, e = tid - rw * 9;
        if (e < 2) sEB[rw * EB_ROW + e * 130] = 0.f;
        else sF0[rw * F0_ROW + (e < 4 ? e - 2 : 127 + e)] = 0.f;
    }
    {   // A0: [mag, re, im] of the new frames
        int tl, f;
        spec_item_first(tid, t_fast, tl, f);
#pragma unroll
        for (int q = 0; q < SPEC_ITEMS; ++q) {
            if (tl < nfr && f < NBINS) {
                const float2 v = spn[q];
                const bool low = f < ERB_LOW;
                float* d = low ? sEB + tl * EB_ROW + 1 + f : sSpec + tl * NBINS + f;
                const int cs = low ? RW * EB_ROW : RW * NBINS;
                d[0] = __builtin_amdgcn_sqrtf(v.x * v.x + v.y * v.y + 1e-12f);
                d[cs] = v.x;
                d[2 * cs] = v.y;
            }
            spec_item_next(t_fast, tl, f);
        }
    }
    // groups B, C, D: behind the consumption of every register load above (see lds_dma_1k)
    constexpr int DMA_B = 1, DMA_C = 2, DMA_D = 4;
    {
        const DmaSeg gb[1] = {{P_ENC + E_BLK, LD::PE + E_BLK, ENC_SIZE - E_BLK}};
        const DmaSeg gc[1] = {{P_GTCN, LD::PG, 2 * GTCN_SIZE}};
        const DmaSeg gd[7] = {{P_DEC + D_BLK + 0 * GBD_SIZE, LD::PD + 0 * GB_SIZE, GB_SIZE},
                              {P_DEC + D_BLK + 1 * GBD_SIZE, LD::PD + 1 * GB_SIZE, GB_SIZE},
                              {P_DEC + D_BLK + 2 * GBD_SIZE, LD::PD + 2 * GB_SIZE, GB_SIZE},
                              {P_DEC + (SPLIT3 ? D_DE3_16 : D_DE3_AE), LD::PD + DL_DE3M, SPLIT3 ? DE3_16_MATS * 256 : 5 * 256},
                              {P_DEC + D_DE3_B, LD::PD + DL_DE, D_BS_W - D_DE3_B},
                              {P_DEC + D_BS_TAB, LD::BS, NBINS * 4},
                              {P_DEC + (SPLIT ? D_DN16 : D_BLK + GB_DN_A), LD::PD + DL_DN, DN_PIECES * 256}};
        static_assert((ENC_SIZE - E_BLK + 255) / 256 <= DMA_B * NW && (2 * GTCN_SIZE + 255) / 256 <= DMA_C * NW, "groups B, C");
        static_assert(3 * ((GB_SIZE + 255) / 256) + (SPLIT3 ? DE3_16_MATS : 5) + (D_BS_W - D_DE3_B + 255) / 256 +
                      (NBINS * 4 + 255) / 256 + DN_PIECES <= DMA_D * NW, "group D");
        lds_dma_group<1, DMA_B, NW>(gb, PF, smem, L.wave, L.lane);
        lds_dma_group<1, DMA_C, NW>(gc, PF, smem, L.wave, L.lane);
        lds_dma_group<7, DMA_D, NW>(gd, PF, smem, L.wave, L.lane);
    }
    wg_barrier_vm<DMA_B + DMA_C + DMA_D>();                        // group A has landed; B, C, D stay in flight
    STAMP(SS, 0)
    {   // A: ERB.bm bands
        const int band = tid & (ERB_BANDS - 1);
        const int lo = sI[I_ERB_LO + band], cnt = sI[I_ERB_N + band];
        float w[ERB_MAXBW];
#pragma unroll
        for (int i = 0; i < ERB_MAXBW; i += 4) {
            const f32x4 t = ld4(sPE + E_ERB_W + band * ERB_MAXBW + i);
            w[i] = t[0]; w[i + 1] = t[1]; w[i + 2] = t[2]; w[i + 3] = t[3];
        }
        for (int ct = tid >> 6; ct < 3 * RW; ct += NW) {
            if ((ct % RW) >= nfr) continue;
            const float* sp = sSpec + ct * NBINS + ERB_LOW + lo;
            float a0 = 0.f, a1 = 0.f;
#pragma unroll
            for (int i = 0; i < ERB_MAXBW; i += 2) {
                a0 += w[i] * (i < cnt ? sp[i] : 0.f);
                a1 += w[i + 1] * (i + 1 < cnt ? sp[i + 1] : 0.f);
            }
            sEB[ct * EB_ROW + 1 + ERB_LOW + band] = a0 + a1;
        }
    }
    wg_barrier();
    STAMP(SS, 1)
    // B: SFE_Lite
    for (int rw = L.wave; rw < 3 * RW; rw += NW) {
        const int tl = rw % RW, c = rw / RW;
        if (tl >= nfr) continue;
        const float w0 = sPE[E_SFE_W + c * 3], w1 = sPE[E_SFE_W + c * 3 + 1], w2 = sPE[E_SFE_W + c * 3 + 2];
        const float* e = sEB + rw * EB_ROW;
        float* d = sF0 + rw * F0_ROW + 2;
        const int f = tid & 63;
        d[f] = w0 * e[f] + w1 * e[f + 1] + w2 * e[f + 2];
        d[f + 64] = w0 * e[f + 64] + w1 * e[f + 65] + w2 * e[f + 66];
        if (f == 0) d[128] = w0 * e[128] + w1 * e[129] + w2 * e[130];
    }
    if (tid < RW * 4 * 4) {                                        // pad positions of E0
        const int r = tid >> 4, cc = (tid >> 2) & 3, gg = tid & 3;
        st4(sE0 + pl(r * ENC_E0_ROW + (cc < 2 ? cc : 65 + cc), gg), splat(0.f));
    }
    wg_barrier();
    STAMP(SS, 2)
    {   // C: en_convs.0; en0 stays in LDS for the decoder tail
        const f32x4 A = ld4(sPE + E_EN0_A + arow(n, g)), Bv = ld4(sPE + E_EN0_B + 4 * g);
        const float a = sPE[E_EN0_S] - 1.0f;
        int off[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int e = 4 * g + s, c = e < 15 ? e / 5 : 0, k = e < 15 ? e % 5 : 0;
            off[s] = c * RW * F0_ROW + k;
        }
        const int nt0 = (nfr * F1 + 15) >> 4;
        for (int tile = L.wave; tile < nt0; tile += NW) {
            const int q = tile * 16 + n;
            int tl = q / F1;
            const int fo = q - tl * F1;
            if (tl >= RW) tl = RW - 1;
            f32x4 bv;
#pragma unroll
            for (int s = 0; s < 4; ++s) bv[s] = sF0[off[s] + tl * F0_ROW + 2 * fo];
            f32x4 acc = mm1<false>(A, bv, Bv);
            acc = prelu4(acc, a);
            st4(sE0 + pl(tl * ENC_E0_ROW + 2 + fo, g), acc);
            if (q < nfr * F1) st4(sEN0 + q * 16 + 4 * g, acc);
        }
    }
    wg_barrier();
    STAMP(SS, 3)
    f32x4 x[1], en1p, en2p, en3p;
    {   // D: en_convs.1; en1 is kept in the slot order of its decoder consumer
        const f32x4 Bv = ld4(sPE + E_EN1_B + 4 * g);
        const float a = sPE[E_EN1_S] - 1.0f;
        const int* ix = sI + I_ENST - ENC_I_SKIP + 0 * 16 + 4 * g;
        x[0] = Bv;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const f32x4 A = ld4(sPE + E_EN1_A + k * 256 + arow(n, g));
            const f32x4 tap = ld4(sE0 + pl(tt.tl[0] * ENC_E0_ROW + 2 * tt.ff[0], g) + k * 16);
            x[0] = mm1<false>(A, tap, x[0]);
        }
        x[0] = prelu4(x[0], a);
        en1p = permute_via_lds(sEB + tt.pp(0) * 16, ix, g, x[0]);
    }
    wg_barrier_vm<DMA_C + DMA_D>();                                // E0 is dead: its region becomes W; group B (block parameters) has landed
    STAMP(SS, 4)
    zero_row_pads<RW, 16, 35>(sWe, tid);
    // GTCN history rows of the lane's position (k_gtcn_ms): requested during the last encoder block
    const int ffl = lane_live ? tt.ff[0] : 0;
    const int tbl = sTB[row];
    f32x4 t1[4], t2[4];
    int r2[4];
    auto fetch_rows = [&](const float* ring) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int d = 1 << k, m2d = 2 * d - 1, row0 = 2 * (d - 1);
            const int r1 = ((row0 + ((tbl + d) & m2d)) * 33 + ffl) * 16 + 4 * g;
            r2[k] = ((row0 + (tbl & m2d)) * 33 + ffl) * 16 + 4 * g;
            t1[k] = ld4(ring + r1);
            t2[k] = ld4(ring + r2[k]);
        }
    };
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        BlockCtx c;
        c.pb = sPE + E_BLK + k * GB_SIZE;
        c.gA = nullptr;
        c.ib = sI + I_ENC_BLK - ENC_I_SKIP + k * 16;
        c.sW = sWe; c.sHk = nullptr; c.sS = sSe; c.sG = sG; c.sEHk = sEHe + k * 16;
        c.sHtop = nullptr; c.sHnext = nullptr;
        c.sE = smem + LD::E;
        c.sY = sG + RW * 16;
        c.nfr = nfr; c.tabs = 0;
        c.sTB = sTB;
        c.ms_roff[0] = (int)(smem + LD::HE - sWe) + row * (2 * 35 * 16);
        c.ms_tb[0] = tbl;
        c.g_hist[0] = STL(0) + ST_ENC_H + ((k * 2 + (tbl & 1)) * 33 + ffl) * 16 + 4 * g;
        if (k < 2) hist_fetch(ST_ENC_H + (k + 1) * 2 * 33 * 16, hv);
        else fetch_rows(STL(0) + ST_G1_H);
        // the next block's history image is written once this block's taps are read (behind its third barrier); every
        // history load has then been consumed before any wave stores a new row in the next block's point_conv1 phase
        gtconv_block<false, 1, true, false, 16, 16, true, 35>(
            x, tt, c, L, [] {}, [&] { if (k < 2) hist_store(smem + LD::HE, std::false_type{}, hv); } STAMP_ARG);
        if (k < 2) {
            const int* ix = sI + I_ENST - ENC_I_SKIP + (k + 1) * 16 + 4 * g;
            const f32x4 y = permute_via_lds(sSe + tt.pp(0) * PERM_RS, ix, g, x[0]);
            if (k == 0) en2p = y; else en3p = y;
        }
        STAMP(SS, 8)
    }
#ifdef GT_STAMPS     // the encoder blocks' phase sums move to slots 10..12: the decoder blocks reuse 5..7
    SS.acc[10] = SS.acc[5]; SS.acc[11] = SS.acc[6]; SS.acc[12] = SS.acc[7];
    SS.acc[5] = SS.acc[6] = SS.acc[7] = 0;
#endif
    // ------------------------------------------------------------------------------------------------- GTCN x 2
    // per position, nothing shared between lanes (k_gtcn_ms); the decoder's first history image is requested now
    hist_fetch(ST_DEC_H, hv);
    // IDX: two of the skips wait out the GTCN in LDS (lane-private 16-byte pieces in the dead encoder images, as in
    // k_stream_wide): the lane pointers of the indexed form are 64-bit -- a slot may sit beyond 4 GB -- and with the rows of
    // four TCN blocks in registers that is what would otherwise go to scratch
    [[maybe_unused]] float* sPark = smem + LD::X + 4 * tid;
    static_assert(2 * NTHR * 4 <= LD::ENC_END - LD::X, "parked skips fit the dead encoder images");
    if constexpr (IDX) {
        st4(sPark, en1p);
        st4(sPark + NTHR * 4, en2p);
    }
    {
        const f32x4 x0 = x[0];
        f32x4 xx = x0;
#pragma unroll
        for (int stack = 0; stack < 2; ++stack) {
            [[maybe_unused]] float* ring = STL(0) + (stack == 0 ? ST_G1_H : ST_G2_H);
            const float* pk = sPG + stack * GTCN_SIZE;
            f32x4 a1[4], a2[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { a1[k] = t1[k]; a2[k] = t2[k]; }
            const int q2[4] = {r2[0], r2[1], r2[2], r2[3]};
            if (stack == 0) fetch_rows(STL(0) + ST_G2_H);
#define RING (IDX ? STL(0) + (stack == 0 ? ST_G1_H : ST_G2_H) : ring)      // (IDX: per block, as every lane pointer)
            tcn_block_ms<1>(xx, pk + 0 * TCN_SIZE, a1[0], a2[0], RING + q2[0], lane_live, n, g);
            tcn_block_ms<2>(xx, pk + 1 * TCN_SIZE, a1[1], a2[1], RING + q2[1], lane_live, n, g);
            tcn_block_ms<4>(xx, pk + 2 * TCN_SIZE, a1[2], a2[2], RING + q2[2], lane_live, n, g);
            tcn_block_ms<8>(xx, pk + 3 * TCN_SIZE, a1[3], a2[3], RING + q2[3], lane_live, n, g);
#undef RING
        }
        x[0] = xx + x0;                                            // gtcn2(gtcn1(x)) + en_outs[4] (Decoder.forward :467)
    }
    if constexpr (IDX) {
        en1p = ld4(sPark);
        en2p = ld4(sPark + NTHR * 4);
        wg_barrier();                                              // every lane has its skips back: the region takes the decoder's images
    }
    STAMP(SS, 9)
    // ------------------------------------------------------------------------------------------------- decoder
    // (k_decoder<false, 1, true, false>: same expressions; skips from registers, en0 from LDS, the spectrogram from spn)
    constexpr int RS = LD::RSD;
    float* sHd = smem + LD::HD;
    float* sW = smem + LD::W;
    float* sS = smem + LD::SD;
    float* sZ = smem + LD::W;
    float* sM = smem + LD::M;
    constexpr int ZS = DEC_ZS;
    // region X is free: every wave that left the encoder's last block is behind that block's closing barrier, i.e. behind
    // all reads of the encoder images.  The first decoder history image is written BEFORE the barrier below, so that
    // every history load has been consumed when the first new row goes out (block 0's point_conv1 phase).
    hist_zero_pads(sHd, RS);
    if constexpr (SPLIT) hist_store(sHd, std::true_type{}, hv);
    else hist_store(sHd, std::false_type{}, hv);
    zero_row_pads<RW, RS>(sW, tid);
    if (tid < 4) sM[2 * RW * F0 + tid] = 0.f;
    wg_barrier();
    STAMP(SS, 13)
    const int npos = nfr * 33;
    f32x4 s0e, s0o;
    auto run_block = [&](int j, const f32x4 skv, auto&& hook, auto&& hook3, auto vmk1) {
        BlockCtx c;
        c.pb = sPD + j * GB_SIZE;
        c.gA = sPD + DL_DN;
        c.ib = sI + I_DEC_BLK - ENC_I_SKIP + j * 16;
        c.sW = sW; c.sHk = nullptr; c.sS = sS; c.sG = sG; c.sEHk = sEHd + j * 16;
        c.sHtop = nullptr; c.sHnext = nullptr;
        c.sE = smem + LD::E;
        c.sY = sG + RW * 16;
        c.nfr = nfr; c.tabs = 0;
        c.sTB = sTB;
        c.ms_roff[0] = (int)(sHd - sW) + row * (2 * 35 * RS);
        c.ms_tb[0] = tbl;
        c.g_hist[0] = STL(0) + ST_DEC_H + ((j * 2 + (tbl & 1)) * 33 + ffl) * 16 + 4 * g;
        gtconv_block<true, 1, true, false, RS, 16, true, 35, 0, decltype(vmk1)::value>(
            x, tt, c, L, [&] { if (j < 2) dense_fetch(j + 1); hook(); }, hook3 STAMP_ARG);
        x[0] = x[0] + skv;
        STAMP(SS, 8)
    };
    // (block j + 1's history rows are requested at the top of block j -- its own image is complete, hv is free -- and
    // land in the image once block j's taps are read; the dense planes of block j + 1 go out by DMA behind block j's dense
    // phase and are waited for at block j + 1's FIRST barrier, one phase before their first reader: see gtconv_block)
    // (first-barrier wait of a block = the vector-memory operations EVERY wave issues behind the DMA of its planes: blocks
    // 0 and 1 the two history loads of the next block; block 2 none -- its wait also takes the live waves' new-row store)
    hist_fetch(ST_DEC_H + 1 * 2 * 33 * 16, hv);
    run_block(0, en3p, [] {},
              [&] { if constexpr (SPLIT) hist_store(sHd, std::true_type{}, hv); else hist_store(sHd, std::false_type{}, hv); },
              std::integral_constant<int, 2>{});
    hist_fetch(ST_DEC_H + 2 * 2 * 33 * 16, hv);
    run_block(1, en2p, [] {},
              [&] { if constexpr (SPLIT) hist_store(sHd, std::true_type{}, hv); else hist_store(sHd, std::false_type{}, hv); },
              std::integral_constant<int, 2>{});
    run_block(2, en1p, [&] {
        // en_outs[0] for the even / odd output bins of the lane's position, from LDS
        const int o0 = (tt.pp(0) < npos ? tt.tl[0] * F1 + 2 * tt.ff[0] : 0) * 16 + 4 * g;
        s0e = ld4(sEN0 + o0);
        s0o = ld4(sEN0 + o0 + (tt.ff[0] < 32 ? 16 : 0));
    }, [] {}, std::integral_constant<int, 0>{});
    // ---- de_convs.3 (gather form) + de_convs.4 (scatter form)
    const int rec3[1] = {o35<RS, 0>(tt, 0, 0)};
    if constexpr (SPLIT3) st_split(sW, rec3[0], g, x[0]);
    else st4(sW + rec3[0] + 4 * g, x[0]);
    wg_barrier();
    f32x4 ze, zo;
    {
        const f32x4 Bv = ld4(sPD + dl(D_DE3_B) + 4 * g);
        const float a = sPD[dl(D_DE3_S)] - 1.0f;
        f32x4 ae1[1], ao1[1];
        de_conv3_tiles<1, SPLIT3, false, RS>(sW, rec3, x, sPD + DL_DE3M, Bv, n, g, ae1, ao1);
        const f32x4 ae = ae1[0], ao = ao1[0];
        const f32x4 A4 = ld4(sPD + dl(D_DE4_A) + arow(n, g));
        f32x4 e2 = prelu4(ae, a), o2 = prelu4(ao, a);
        e2 = e2 + s0e;
        o2 = o2 + s0o;
        ze = mm1<false>(A4, e2, splat(0.f));
        zo = mm1<false>(A4, o2, splat(0.f));
    }
    wg_barrier();                                                  // region W becomes Z
    if (g < 3) {
        st4(sZ + (tt.tl[0] * DEC_Z_ROW + 1 + 2 * tt.ff[0]) * ZS + 4 * g, ze);
        if (tt.ff[0] < 32) st4(sZ + (tt.tl[0] * DEC_Z_ROW + 2 + 2 * tt.ff[0]) * ZS + 4 * g, zo);
    }
    if (tid < RW * 2 * 4 && (tid & 3) < 3)
        st4(sZ + ((tid >> 3) * DEC_Z_ROW + ((tid >> 2) & 1) * (DEC_Z_ROW - 1)) * ZS + 4 * (tid & 3), splat(0.f));
    wg_barrier();
    {   // de_convs.4 gather + BN + Tanh
        static_assert(4 * F0 <= NTHR && RW % 2 == 0, "two threads per (o, f'')");
        if (tid < 4 * F0) {
            const int h = tid >= 2 * F0 ? 1 : 0, c = tid - h * 2 * F0, o = c >= F0 ? 1 : 0, fq = c - o * F0;
            const int par = fq & 1, m = fq >> 1;
            const float* zr = sZ + (h * DEC_Z_ROW + 1 + m) * ZS;
            const float* r1 = zr + ZS + o * 5 + par;
            const float* r2p = zr + o * 5 + 2 + par;
            const float* r3 = zr - ZS + (par ? 10 : o * 5 + 4);
            const float bias = sPD[dl(D_DE4_B) + o];
            float* mo = sM + (o * RW + h) * F0 + fq;
#pragma unroll
            for (int j = 0; j < RW / 2; ++j) {
                constexpr int ZF = 2 * DEC_Z_ROW * ZS;
                const float sum = bias + r1[j * ZF] + r2p[j * ZF] + r3[j * ZF];
                mo[j * 2 * F0] = fast_tanh(sum);
            }
        }
    }
    wg_barrier();
    STAMP(SS, 14)
    {   // ERB.bs + complex ratio mask + output layout
        int tq, f;
        spec_item_first(tid, t_fast, tq, f);
        float* obase = out + (long)b * NS * osb;
        const int osf32 = (int)osf, ost32 = (int)osb;
        constexpr int GRP = 3;
        static_assert(SPEC_ITEMS % GRP == 0, "mask items come in groups of three");
#pragma unroll
        for (int q0 = 0; q0 < SPEC_ITEMS; q0 += GRP) {
            bool ok[GRP];
            int fo[GRP];
            const float* m0[GRP];
            f32x4 tb[GRP];
#pragma unroll
            for (int j = 0; j < GRP; ++j) {
                ok[j] = tq < nfr && f < NBINS;
                const int fc = ok[j] ? f : 0, tc = ok[j] ? tq : 0;
                tb[j] = ld4(sBS + fc * 4);
                m0[j] = sM + tc * F0;
                fo[j] = f * osf32 + tq * ost32;
                spec_item_next(t_fast, tq, f);
            }
            float a0[GRP], a1[GRP], b0[GRP], b1[GRP];
#pragma unroll
            for (int j = 0; j < GRP; ++j) {
                const float* mp = m0[j] + __float_as_int(tb[j][0]);
                a0[j] = mp[0]; a1[j] = mp[1]; b0[j] = mp[RW * F0]; b1[j] = mp[RW * F0 + 1];
            }
#pragma unroll
            for (int j = 0; j < GRP; ++j) {
                const bool two = tb[j][2] != 0.f;
                const float mr = tb[j][1] * a0[j] + (two ? tb[j][2] * a1[j] : 0.f);
                const float mi = tb[j][1] * b0[j] + (two ? tb[j][2] * b1[j] : 0.f);
                const float re = spn[q0 + j].x, im = spn[q0 + j].y;
                const float yr = re * mr - im * mi, yi = im * mr + re * mi;
                if (ok[j]) *reinterpret_cast<float2*>(obase + fo[j]) = make_float2(yr, yi);
            }
        }
    }
    // ------------------------------------------------------------------------------------------------- epilogue
    // energy rings and frame counters (the h rows and the TCN rows went out where they were produced)
    if (tid < nlive * 48) {
        const int sidx = tid / 48, e = tid - sidx * 48;
        stb[SROW(sidx) + ST_ENC_E + e] = sEHe[tid];
        stb[SROW(sidx) + ST_DEC_E + e] = sEHd[tid];
    }
    if (tid < nlive) reinterpret_cast<int*>(stb + SROW(tid))[0] = (sTB[tid] + 1) & 0xFFFF;
    STAMP(SS, 15)
    STAMP_OUT(SS, stamps)
