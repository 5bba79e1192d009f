// Included into the body of a kernel (gemm_fp8.hip): gemm_fp8_mfma / gemm_fp8_mfma_tr, one tile.  The kernel provides p, WM, WN, TM, TN, EPI, K64, MX and TR.
    constexpr int NWAVES = WM * WN;
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN, ROWS = BM + BN, NLD = ROWS / (8 * NWAVES);
    static_assert(ROWS % (8 * NWAVES) == 0 && BM % 8 == 0, "DMA pieces must split evenly over the waves");
    extern __shared__ __attribute__((aligned(128))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int c32 = lane & 31, h = lane >> 5;

    const int nbn = (p.N + BN - 1) / BN, nbm = (p.M + BM - 1) / BM;
    const int ntiles = nbm * nbn;
    int tile;
    {
        const int bid = blockIdx.x, xcd = bid & 7, idx = bid >> 3, qq = ntiles >> 3, rr = ntiles & 7;
        tile = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + idx;
    }
    const int m0 = (tile / nbn) * BM, n0 = (tile % nbn) * BN;

    unsigned src[NLD];   // byte (= element) offsets
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
        const int row = 8 * (wave + NWAVES * u) + (lane >> 3);
        const int c = (lane & 7) ^ ((row >> 1) & 7);
        if (8 * (wave + NWAVES * u) < BM) {
            int gm = m0 + row;
            gm = gm < p.M ? gm : p.M - 1;
            src[u] = (unsigned)gm * (unsigned)p.lda + c * 16;
        } else {
            int gn = n0 + row - BM;
            gn = gn < p.N ? gn : p.N - 1;
            src[u] = (unsigned)gn * (unsigned)p.K + c * 16;
        }
    }
    auto issue = [&](int stage, int k0) {
        // the k-tile's advance travels in a scalar base, the lane's row / chunk offset is the kernel constant src[u]: no vector address
        // arithmetic per piece (`global_load_lds_dwordx4 voff, s[base]`; invisible to hipcc's waitcnt pass - every hand-over below
        // carries its explicit s_waitcnt vmcnt)
        const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)((__attribute__((address_space(3))) char *)(smem + stage * (ROWS * ROW8))));
        const unsigned char *abase = p.A + k0, *wbase = p.W + k0;
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int piece = wave + NWAVES * u;
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep)
                         : "v"(src[u]), "s"(8 * piece < BM ? abase : wbase), "s"(dst + piece * 1024)
                         : "memory");
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    const int sw = (c32 >> 1) & 7;
    const int nk = p.K / BKE;
    const int a_row = (wm * TM * 32 + c32) * ROW8, b_row = (BM + wn * TN * 32 + c32) * ROW8;

    if constexpr (!K64) {
        auto load_frags = [&](int stage, int c, i64x2(&xa)[TM], i64x2(&wb)[TN]) {
            const char *base = smem + stage * (ROWS * ROW8) + ((c * 2 + h) ^ sw) * 16;
#pragma unroll
            for (int i = 0; i < TM; ++i) xa[i] = *reinterpret_cast<const i64x2 *>(base + a_row + i * 32 * ROW8);
#pragma unroll
            for (int j = 0; j < TN; ++j) wb[j] = *reinterpret_cast<const i64x2 *>(base + b_row + j * 32 * ROW8);
        };
        auto mfma_chunk = [&](const i64x2(&xa)[TM], const i64x2(&wb)[TN]) {
#pragma unroll
            for (int half = 0; half < 2; ++half)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(wb[j][half], xa[i][half], acc[i][j], 0, 0, 0);
        };
        i64x2 xa0[TM], wb0[TN], xa1[TM], wb1[TN];
        issue(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // explicit: the first tile has landed before anybody reads it
        __syncthreads();
        load_frags(0, 0, xa0, wb0);
        // (round 4: the order reads | MFMAs is pinned with sched_barrier - left alone, the scheduler sinks a chunk's reads behind its
        //  MFMAs, right in front of the wait that needs them: profiles/r04_tr_pinned_order_ab.txt, same finding as gemm_bf16_tr)
        for (int kt = 0; kt < nk; ++kt) {
            const int cur = kt & 1;
            const int knext = (kt + 1 < nk ? kt + 1 : nk - 1) * BKE;
            load_frags(cur, 1, xa1, wb1);
            __builtin_amdgcn_sched_barrier(0);
            issue(cur ^ 1, knext);
            mfma_chunk(xa0, wb0);
            __builtin_amdgcn_sched_barrier(0);
            load_frags(cur, 2, xa0, wb0);
            __builtin_amdgcn_sched_barrier(0);
            mfma_chunk(xa1, wb1);
            __builtin_amdgcn_sched_barrier(0);
            load_frags(cur, 3, xa1, wb1);
            __builtin_amdgcn_sched_barrier(0);
            mfma_chunk(xa0, wb0);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // explicit: do not rely on hipcc to drain the LDS-DMA in front of the barrier
            __syncthreads();   // hand-over: tile kt+1 landed in every wave, stage cur released
            load_frags(cur ^ 1, 0, xa0, wb0);
            __builtin_amdgcn_sched_barrier(0);
            mfma_chunk(xa1, wb1);
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        // MX: sx / sw = the scale dwords of tile kt (shifted: byte 0 = block h, byte 2 = block 2 + h), nx / nw_ = tile kt + 1 in flight
        unsigned xo[MX ? TM : 1], wo[MX ? TN : 1], sx[MX ? TM : 1], sw_[MX ? TN : 1], nx[MX ? TM : 1], nw_[MX ? TN : 1];
        const unsigned sh = 8u * (unsigned)h;
        if constexpr (MX) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int r = m0 + wm * TM * 32 + i * 32 + c32;
                xo[i] = (unsigned)(r < p.M ? r : p.M - 1) * (unsigned)p.ldas;
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int r = n0 + wn * TN * 32 + j * 32 + c32;
                wo[j] = (unsigned)(r < p.N ? r : p.N - 1) * (unsigned)p.ldws;
            }
        }
        // (hand-counted like the DMA: hipcc cannot see these loads, the registers are read only behind an explicit vmcnt wait
        //  that names them - `landed`)
        auto fetch_scales = [&](unsigned(&dx)[MX ? TM : 1], unsigned(&dw)[MX ? TN : 1], int kt) {
            if constexpr (MX) {
                const unsigned char *xb = p.As + 4 * kt, *wbs = p.Ws + 4 * kt;
#pragma unroll
                for (int i = 0; i < TM; ++i) asm volatile("global_load_dword %0, %1, %2" : "=v"(dx[i]) : "v"(xo[i]), "s"(xb) : "memory");
#pragma unroll
                for (int j = 0; j < TN; ++j) asm volatile("global_load_dword %0, %1, %2" : "=v"(dw[j]) : "v"(wo[j]), "s"(wbs) : "memory");
            }
        };
        auto landed = [&](unsigned(&dx)[MX ? TM : 1], unsigned(&dw)[MX ? TN : 1]) {   // behind a vmcnt that covers them
            if constexpr (MX) {
#pragma unroll
                for (int i = 0; i < TM; ++i) { asm volatile("" : "+v"(dx[i])); sx[i] = dx[i] >> sh; }
#pragma unroll
                for (int j = 0; j < TN; ++j) { asm volatile("" : "+v"(dw[j])); sw_[j] = dw[j] >> sh; }
            }
        };
        auto mfma_chunk = [&](const i32x8(&xa)[TM], const i32x8(&wb)[TN], auto chunk) {
            constexpr int OPS = 2 * decltype(chunk)::value;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if constexpr (MX)
                        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wb[j], xa[i], acc[i][j], 0, 0, OPS, (int)sw_[j], OPS, (int)sx[i]);
                    else
                        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wb[j], xa[i], acc[i][j], 0, 0, 0, 0, 0, 0);
                }
        };
        const std::integral_constant<int, 0> chunk0{};
        const std::integral_constant<int, 1> chunk1{};
        i32x8 xa0[TM], wb0[TN], xa1[TM], wb1[TN];
        // Round 3: the DMA of tile kt+2 is issued right BEHIND the hand-over barrier of iteration kt (stage `cur` is free there:
        // every wave's last fragments of tile kt are in registers) and waited for at the NEXT hand-over - a whole k-tile of MFMA
        // time (2048 cycles per SIMD) to land.  Rounds 1-2 issued tile kt+1 at the top of iteration kt and waited for it half a
        // k-tile later: shorter than an L2 / Infinity-Cache round trip under load, so every k-tile stalled on its own DMA.
        // Round 4: the order reads | DMA pieces | MFMAs | wait is PINNED (sched_barrier), and for that every fragment read is an asm
        // statement waited for by hand.  Left to hipcc, a chunk's reads sank behind its MFMAs - right in front of the wait that needs
        // them, so the wait in front of the hand-over barrier and the first MFMA of the next chunk each sat out an LDS latency - and
        // its own counted waits degenerated to lgkmcnt(0) right behind freshly issued reads (it cannot see across the asm DMA).
        // The 320-row tile keeps hipcc's order: both fragment sets live at once (112 registers beside 160 of accumulators) do not
        // fit, which is why the reads were sunk there in the first place.
        constexpr bool PIN = TM < 5;
        // fragment of rows r: chunks (4 c + 2 h) ^ sw and (4 c + 2 h + 1) ^ sw of the 128-byte row - the chunk index is an XOR of
        // address bits 6 (c) and 4 (second half); every other term is a multiple of 128 bytes (aligned(128) stage memory)
        // MX: the fragment of chunk c is 16-B chunks (4 c + h) ^ sw and (4 c + 2 + h) ^ sw instead - the instruction's block b of a
        // 64-deep step is the b-th 16 bytes of BOTH lane halves, so that block b = the row's 32 consecutive bytes 64 c + 32 b
        const unsigned lds0 = (unsigned)(uintptr_t)((__attribute__((address_space(3))) char *)smem);
        constexpr unsigned HI = MX ? 32u : 16u;
        const int hc = MX ? h : 2 * h;
        const unsigned fa0 = lds0 + a_row + ((hc ^ sw) << 4), fb0 = lds0 + b_row + ((hc ^ sw) << 4);
        auto load_frags = [&](int stage, int c, i32x8(&xa)[TM], i32x8(&wb)[TN]) {
            if constexpr (PIN) {
                const unsigned so = (unsigned)(stage * (ROWS * ROW8));
                const unsigned a_lo = (fa0 + so) ^ (unsigned)(c << 6), a_hi = a_lo ^ HI, b_lo = (fb0 + so) ^ (unsigned)(c << 6), b_hi = b_lo ^ HI;
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    union { i32x4 v[2]; i32x8 f; } u;
                    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(u.v[0]) : "v"(a_lo), "n"(i * 32 * ROW8));
                    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(u.v[1]) : "v"(a_hi), "n"(i * 32 * ROW8));
                    xa[i] = u.f;
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    union { i32x4 v[2]; i32x8 f; } u;
                    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(u.v[0]) : "v"(b_lo), "n"(j * 32 * ROW8));
                    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(u.v[1]) : "v"(b_hi), "n"(j * 32 * ROW8));
                    wb[j] = u.f;
                }
            } else {
                const char *base = smem + stage * (ROWS * ROW8);
                const int o0 = MX ? ((4 * c + h) ^ sw) * 16 : ((4 * c + 2 * h) ^ sw) * 16;
                const int o1 = MX ? ((4 * c + 2 + h) ^ sw) * 16 : ((4 * c + 2 * h + 1) ^ sw) * 16;
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const i32x4 lo = *reinterpret_cast<const i32x4 *>(base + a_row + i * 32 * ROW8 + o0);
                    const i32x4 hi = *reinterpret_cast<const i32x4 *>(base + a_row + i * 32 * ROW8 + o1);
                    xa[i] = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const i32x4 lo = *reinterpret_cast<const i32x4 *>(base + b_row + j * 32 * ROW8 + o0);
                    const i32x4 hi = *reinterpret_cast<const i32x4 *>(base + b_row + j * 32 * ROW8 + o1);
                    wb[j] = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                }
            }
        };
        // (PIN: every group below is fenced; else the fences and hand waits for the reads drop out and hipcc orders / waits as before)
        auto fence = [&]() { if constexpr (PIN) __builtin_amdgcn_sched_barrier(0); };
        auto reads_done = [&]() { if constexpr (PIN) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); };
        if constexpr (MX) fetch_scales(nx, nw_, 0);
        issue(0, 0);
        issue(1, (nk > 1 ? 1 : 0) * BKE);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLD) : "memory");      // tile 0 landed; tile 1's NLD pieces stay in flight
        landed(nx, nw_);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        load_frags(0, 0, xa0, wb0);
        reads_done();
        fence();
        for (int kt = 0; kt < nk; ++kt) {
            const int cur = kt & 1;
            const int k2 = (kt + 2 < nk ? kt + 2 : nk - 1) * BKE;
            load_frags(cur, 1, xa1, wb1);
            fence();
            mfma_chunk(xa0, wb0, chunk0);
            fence();
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // tile kt+1 landed; own reads of stage cur retired
            __builtin_amdgcn_s_barrier();   // hand-over: tile kt+1 visible to every wave, stage cur released
            asm volatile("" ::: "memory");
            fence();
            if constexpr (PIN) {
                load_frags(cur ^ 1, 0, xa0, wb0);
                fence();
                if constexpr (MX) fetch_scales(nx, nw_, kt + 1 < nk ? kt + 1 : nk - 1);
                issue(cur, k2);             // tile kt+2 -> stage cur (a clamped re-fetch on the last two iterations, never read)
            } else {
                if constexpr (MX) fetch_scales(nx, nw_, kt + 1 < nk ? kt + 1 : nk - 1);
                issue(cur, k2);
                load_frags(cur ^ 1, 0, xa0, wb0);
            }
            mfma_chunk(xa1, wb1, chunk1);
            fence();
            reads_done();
            if constexpr (MX) {
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLD) : "memory");   // tile kt+1's scales; tile kt+2's pieces stay in flight
                landed(nx, nw_);
            }
            fence();
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the clamped re-fetches must not outlive the LDS allocation
    }

    const bool cols_in = (n0 + BN <= p.N) && ((p.ldy & 3) == 0);
    const int mw = m0 + wm * TM * 32, nw = n0 + wn * TN * 32;
    // (the slab path stores eight bf16 columns per lane - EPI_BIAS, the q|k|v output -: ldy a multiple of 8 then)
    if (cols_in && (EPI != EPI_BIAS || (p.ldy & 7) == 0) && m0 + BM <= p.M && !p.direct_epi && !(MX && EPI == EPI_BIAS_GELU)) {
        __syncthreads();     // every wave is out of the k-loop (and its DMA drained): the stage memory becomes slab buffers
        const float ab = p.d_act ? p.d_act[0] : p.ab_scale;
        const float oinv = (EPI == EPI_BIAS_GELU && p.d_out) ? 1.0f / p.d_out[0] : p.out_inv_scale;
        if constexpr (TR) {
            GemmExtra x{};
            x.Ypre = ypre_of(p); x.rowscale = rowscale_of(p);
            store_rows_via_lds<TM, TN, EPI, EPI == EPI_SCALE_RESID ? EPI_OUT_F32 : EPI == EPI_BIAS_GELU ? EPI_OUT_FP8 : EPI_OUT_BF16>(
                acc, smem + wave * EPI_WAVE_BYTES, p.Y, p.Y2, p.R, p.bias, p.lam, p.d_wrow, p.ldy, mw, nw, lane, ab, oinv, x);
        } else
        store_rows_via_lds<TM, TN, EPI, EPI == EPI_SCALE_RESID ? EPI_OUT_F32 : EPI == EPI_BIAS_GELU ? EPI_OUT_FP8 : EPI_OUT_BF16>(
            acc, smem + wave * EPI_WAVE_BYTES, p.Y, p.Y2, p.R, p.bias, p.lam, p.d_wrow, p.ldy, mw, nw, lane, ab, oinv);
    } else if (cols_in && m0 + BM <= p.M) store_q<TM, TN, EPI, 0, MX, TR>(p, acc, mw, nw, lane);
    else if (cols_in) store_q<TM, TN, EPI, 1, MX, TR>(p, acc, mw, nw, lane);
    else store_q<TM, TN, EPI, 2, MX, TR>(p, acc, mw, nw, lane);
