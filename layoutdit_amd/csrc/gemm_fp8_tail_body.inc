// Included into the body of a kernel (gemm_fp8.hip): gemm_fp8_tail / gemm_fp8_tail_tr, one 32 x 32 tile of the tail.  The kernel provides p, EPI, MX and TR.
    constexpr int D = 4;
    const int lane = threadIdx.x, c32 = lane & 31, h = lane >> 5;
    const int nct = (p.N + 31) / 32;
    const int n0 = (blockIdx.x % nct) * 32, m0 = (blockIdx.x / nct) * 32;
    const int ra = m0 + c32 < p.M ? m0 + c32 : p.M - 1, rw = n0 + c32 < p.N ? n0 + c32 : p.N - 1;
    // (MX: the two 16-byte halves of a lane's operand are bytes 16 h and 32 + 16 h of the step - see gemm_fp8_mfma)
    constexpr int HO = MX ? 32 : 16;
    const unsigned char *ap = p.A + (size_t)ra * p.lda + (MX ? 16 : 32) * h, *wp = p.W + (size_t)rw * p.K + (MX ? 16 : 32) * h;
    const int nsteps = p.K / 64;
    f32x16 acc[1][1];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[0][0][e] = 0.0f;
    i32x8 xa0[D], wb0[D], xa1[D], wb1[D];
    int sa0[D], sb0[D], sa1[D], sb1[D];
    const unsigned char *asp = MX ? p.As + (size_t)ra * p.ldas + h : nullptr, *wsp = MX ? p.Ws + (size_t)rw * p.ldws + h : nullptr;
    auto lds_ = [&](int(&sa)[D], int(&sb)[D], int s0) {
        if constexpr (MX)
#pragma unroll
            for (int u = 0; u < D; ++u) {
                const int s = s0 + u < nsteps ? s0 + u : nsteps - 1;
                sa[u] = asp[2 * s];
                sb[u] = wsp[2 * s];
            }
    };
    auto ld = [&](i32x8(&xa)[D], i32x8(&wb)[D], int s0) {
#pragma unroll
        for (int u = 0; u < D; ++u) {
            const int s = s0 + u < nsteps ? s0 + u : nsteps - 1;
            const i32x4 al = *reinterpret_cast<const i32x4 *>(ap + 64 * s), ah = *reinterpret_cast<const i32x4 *>(ap + 64 * s + HO);
            const i32x4 wl = *reinterpret_cast<const i32x4 *>(wp + 64 * s), wh = *reinterpret_cast<const i32x4 *>(wp + 64 * s + HO);
            xa[u] = i32x8{al[0], al[1], al[2], al[3], ah[0], ah[1], ah[2], ah[3]};
            wb[u] = i32x8{wl[0], wl[1], wl[2], wl[3], wh[0], wh[1], wh[2], wh[3]};
        }
    };
    auto mm = [&](const i32x8(&xa)[D], const i32x8(&wb)[D], const int(&sa)[D], const int(&sb)[D], int s0) {
#pragma unroll
        for (int u = 0; u < D; ++u)
            if (s0 + u < nsteps) {
                if constexpr (MX)
                    acc[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wb[u], xa[u], acc[0][0], 0, 0, 0, sb[u], 0, sa[u]);
                else
                    acc[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wb[u], xa[u], acc[0][0], 0, 0, 0, 0, 0, 0);
            }
    };
    ld(xa0, wb0, 0);
    lds_(sa0, sb0, 0);
    for (int s0 = 0; s0 < nsteps; s0 += 2 * D) {
        ld(xa1, wb1, s0 + D);
        lds_(sa1, sb1, s0 + D);
        mm(xa0, wb0, sa0, sb0, s0);
        ld(xa0, wb0, s0 + 2 * D);
        lds_(sa0, sb0, s0 + 2 * D);
        mm(xa1, wb1, sa1, sb1, s0 + D);
    }
    if ((n0 + 32 <= p.N) && ((p.ldy & 3) == 0)) store_q<1, 1, EPI, 1, MX, TR>(p, acc, m0, n0, lane);
    else store_q<1, 1, EPI, 2, MX, TR>(p, acc, m0, n0, lane);
