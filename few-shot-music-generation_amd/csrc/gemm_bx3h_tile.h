// One (row tile tm, column tile tn, K slab z) item of the 256 x 256-tile kernel: everything behind the choice of the item -- operand
// staging, the k loop, column sums, the store epilogue.  NOT a header: a fragment of a kernel's body, included by gemm.hip where a kernel
// has chosen its item -- k_gemm_bx3h (one GEMM) and k_gemm_bx3h_pair (the work lists of two), which therefore run the same statements.
// The including scope provides: g (GemmArgs), tm, tn, z; AMODE, BMODE, PROF, BUFM, AG, EM and XT, PLANE, OPER, DMA, A_BYTES, PIPE as
// constants; smem, s_cs (LDS); tid, lane, wave, late, l31, khalf; the BX_STAMP macro.
    const int m0 = tm * XT, n0 = tn * XT;
    // wave tile: rows 128 wm ..., columns 64 wn ... of the block tile (gemm_edge.h: wave >> 2, wave & 3 unless an edge tile has at most
    // four live sub-tiles and the plain map would pair them on a SIMD).  `wave` itself stays what everything about STAGING goes by.
    const GemmEdgeWave ew = gemm_edge_wave(min(XT, g.M - m0), min(XT, g.N - n0), wave);
    const int wm = __builtin_amdgcn_readfirstlane(ew.wm), wn = __builtin_amdgcn_readfirstlane(ew.wn);
    // wave-uniform, in an SGPR: a dead wave skips the fragment reads and the MFMAs of the k loop and nothing else -- its share of the
    // staging, every barrier and the epilogue of its sub-tile (zero accumulators; what it stores or leaves as a softmax partial never
    // depended on them: rows >= M and columns >= N are masked there) stay where they are
    const bool live = __builtin_amdgcn_readfirstlane((int)ew.live) != 0;
    unsigned long long pacc[5] = {0, 0, 0, 0, 0}, plast = 0, p_entry = 0, p_loop = 0;
    if (PROF) { p_entry = plast = __builtin_amdgcn_s_memtime(); }

    int kb = 0, ke = g.K;
    if (g.ksplit > 1) {
        const int per = ((g.K + g.ksplit - 1) / g.ksplit + 15) / 16 * 16;
        kb = z * per;
        ke = min(g.K, kb + per);
    }
    const int nk = (ke > kb) ? (ke - kb + 15) / 16 : 0;
    const int nfull = (ke > kb) ? (ke - kb) / 16 : 0;

    typename BxStagerSel<DMA, AMODE, XT, 512, (BUFM >= 2), AG>::type sa;      // 512 threads cover 256 rows / columns, 8 values each
    typename BxStagerSel<DMA, BMODE, XT, 512, (BUFM >= 1)>::type sb;
    if constexpr (AG) {                              // which part of op(A) this row tile belongs to
        static_assert(!AG || (DMA && AMODE == OP_XC), "two-part A: LDS-DMA staged x-contiguous operand");
        const bool first = m0 < g.m_split;
        sa.init(first ? g.A : g.A2, first ? g.lda : g.lda2, first ? g.m_split : g.M - g.m_split, first ? m0 : m0 - g.m_split,
                first ? g.gather : nullptr, kb, tid, g.K, smem + PIPE + wave * 2048, ke);
    } else
    if constexpr (DMA && AMODE == OP_XC) sa.init(g.A, g.lda, g.M, m0, nullptr, kb, tid, g.K, smem + PIPE + wave * 2048);
    else sa.init(g.A, g.lda, g.M, m0, g.gather, kb, tid, g.K);
    if constexpr (DMA && BMODE == OP_XC) sb.init(g.B, g.ldb, g.N, n0, nullptr, kb, tid, g.K, smem + PIPE + ((AMODE == OP_XC) ? 8 * 2048 : 0) + wave * 2048);
    else sb.init(g.B, g.ldb, g.N, n0, nullptr, kb, tid, g.K);

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // column sums of op(B): thread = (x = tid % 256, k half = tid / 256) of the XC stager
    const bool do_colsum = (BMODE == OP_XC) && g.colsum != nullptr && tm == 0;
    float csum = 0.0f;
    // weighted column sums (GemmArgs::colsum_w): ONE dword load per wave and k tile -- lane l takes the weight of K row 8 * (its k half)
    // + l % 8, requested with the tile's loads a k tile ahead -- and the commit's eight FMAs read it through DPP row broadcasts
    // (row_newbcast:j: lane j of the own row of 16).  What was measured against it on the 400 us dW launch: two float4 loads per lane at
    // the commit +46 us (latency in the open), the same a k tile ahead +130 us (two more 1 KiB vector loads per wave beside the four of
    // the LDS-DMA staging; a CU issues one wave-level load per ~20 cycles), s_load_dwordx16 through the scalar cache +46 us (an SMEM
    // request in flight turns every counted LDS wait of the k loop and its barrier into lgkmcnt(0)).  The request is UNCONDITIONAL in
    // the kernels that can be asked for weights (both operands x-contiguous: the weight-gradient shapes); a launch without weights reads
    // floats of B it never uses.
    constexpr bool WCS = AMODE == OP_XC && BMODE == OP_XC;
    const bool cs_weighted = WCS && do_colsum && g.colsum_w != nullptr;
    const float* cs_p = (WCS && g.colsum_w != nullptr ? g.colsum_w : g.B) + kb + 8 * ((DMA && BMODE == OP_XC) ? (lane >> 5) : (tid >> 8)) + (lane & 7);
    float cs_wv = 0.0f;
    unsigned char* const smemB = smem + A_BYTES;
#define BXH_FETCH(T)                                                                                           \
    if ((T) < nfull) { sa.fetch(); sb.fetch(); }                                                               \
    else { sa.fetch_partial(kb + (T) * 16, ke, tid); sb.fetch_partial(kb + (T) * 16, ke, tid); }               \
    if constexpr (WCS) cs_wv = cs_p[(T) * 16];
#define BXH_COMMIT(ST)                                                                                         \
    sa.load();                                                                                                 \
    sb.load();                                                                                                 \
    if (do_colsum) {                                                                                           \
        if (cs_weighted) {               /* weighted per K row: cs_wv came in with this tile's loads (BXH_FETCH) */ \
            csum = fmaf(sb.v[0], cs_bcast<0>(cs_wv), csum); csum = fmaf(sb.v[1], cs_bcast<1>(cs_wv), csum);   \
            csum = fmaf(sb.v[2], cs_bcast<2>(cs_wv), csum); csum = fmaf(sb.v[3], cs_bcast<3>(cs_wv), csum);   \
            csum = fmaf(sb.v[4], cs_bcast<4>(cs_wv), csum); csum = fmaf(sb.v[5], cs_bcast<5>(cs_wv), csum);   \
            csum = fmaf(sb.v[6], cs_bcast<6>(cs_wv), csum); csum = fmaf(sb.v[7], cs_bcast<7>(cs_wv), csum);   \
        } else csum += sb.sum8();                                                                              \
    }                                                                                                          \
    sa.commit(smem + (ST) * OPER);                                                                             \
    sb.commit(smemB + (ST) * OPER);

    if (nk > 0) {
        BXH_FETCH(0)
        BXH_COMMIT(0)
        if (nk > 1) { BXH_FETCH(1) }                      // every fetch sits right behind a commit (the VALU half of an iteration)
    }
    bx_barrier();
    const int fa = khalf * (XT * 16) + (wm * 128 + l31) * 16, fb = khalf * (XT * 16) + (wn * 64 + l31) * 16;
    if (PROF) { p_loop = plast = __builtin_amdgcn_s_memtime(); }
    // A wave whose sub-tile lies outside M x N has a k loop of its own: its share of the staging and the barrier of every k tile, no
    // fragment reads, no MFMAs -- the LDS path and the matrix pipe of its SIMD belong to the live wave beside it.  (A branch around the
    // reads and the MFMAs inside ONE loop made them basic blocks of their own: the early waves' split no longer interleaved with
    // their MFMAs, 16-18 more VGPRs.  The live loop below is the loop as it was.)  Early or late makes no difference without MFMAs.
    if (!live) {
        for (int kt = 0; kt < nk; ++kt) {
            if (kt + 1 < nk) {
                BXH_COMMIT((kt + 1) & 1)
                if (kt + 2 < nk) { BXH_FETCH(kt + 2) }
            }
            bx_barrier();
        }
    } else
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;
        // every wave starts with the fragments of the FIRST term (a[2], b[0]: 6 of the 18 reads), so that the late waves'
        // first MFMAs do not wait for LDS behind their commit; the other twelve follow the commit and land behind those
        // MFMAs.  (All 18 up front cost 72 live registers during the split: 10 spilled with two x-contiguous operands, and
        // the stagers' load offsets spilled -- reloaded from scratch in front of every load -- with LDS-DMA.)  Two
        // k-contiguous operands have the registers for all 18 and are faster that way (3670 against 3970 cycles per k tile).
        constexpr bool READS_ALL_FIRST = AMODE == OP_KC && BMODE == OP_KC;
        const unsigned char* at = smem + (kt & 1) * OPER;
        const unsigned char* bt = smemB + (kt & 1) * OPER;
        bf16x8_t a[3][4], b[3][2];
#define BXH_READ_A(pl) _Pragma("unroll") for (int i = 0; i < 4; ++i) a[pl][i] = *reinterpret_cast<const bf16x8_t*>(at + (pl) * PLANE + fa + i * 512);
#define BXH_READ_B(pl) _Pragma("unroll") for (int j = 0; j < 2; ++j) b[pl][j] = *reinterpret_cast<const bf16x8_t*>(bt + (pl) * PLANE + fb + j * 512);
        BXH_READ_A(2) BXH_READ_B(0)
        if (READS_ALL_FIRST) { BXH_READ_A(0) BXH_READ_B(2) BXH_READ_A(1) BXH_READ_B(1) }
        __builtin_amdgcn_sched_barrier(0);
        if (late && more) {
            BXH_COMMIT((kt + 1) & 1)
            if (kt + 2 < nk) { BXH_FETCH(kt + 2) }
        }
        __builtin_amdgcn_sched_barrier(0);
        BX_STAMP(3)
        if (!READS_ALL_FIRST) { BXH_READ_A(0) BXH_READ_B(2) BXH_READ_A(1) BXH_READ_B(1) }
#undef BXH_READ_A
#undef BXH_READ_B
#define BXH_TERM(PA, PB)                                                                                       \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                          \
        _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                          \
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PA][i], b[PB][j], acc[i][j], 0, 0, 0);
        BXH_TERM(2, 0) BXH_TERM(0, 2) BXH_TERM(1, 1) BXH_TERM(1, 0) BXH_TERM(0, 1) BXH_TERM(0, 0)
#undef BXH_TERM
        BX_STAMP(2)
        if (!late && more) {
            BXH_COMMIT((kt + 1) & 1)
            if (kt + 2 < nk) { BXH_FETCH(kt + 2) }
        }
        BX_STAMP(3)
        bx_barrier();
        BX_STAMP(4)
    }
#undef BXH_FETCH
#undef BXH_COMMIT
    const unsigned long long p_exit_loop = PROF ? __builtin_amdgcn_s_memtime() : 0;

    if (do_colsum) {                    // the two k halves of a column live in threads tid and tid + 256 (LDS-DMA: lanes l, l + 32)
        const int col = (DMA && BMODE == OP_XC) ? 32 * wave + (lane & 31) : (tid & 255);
        const bool upper = (DMA && BMODE == OP_XC) ? lane >= 32 : tid >= 256;
        if (upper) s_cs[col] = csum;
        bx_barrier();
        if (!upper && n0 + col < g.N) g.colsum[(long long)z * g.colsum_slab + n0 + col] = csum + s_cs[col];
    }
    float* ep = reinterpret_cast<float*>(smem) + wave * (32 * 68);
    if (PROF && (g.dbg & 8)) {          // experiment: no output (what the store tail costs)
        float sink = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) sink += acc[i][j][r];
        if (sink == 1.2345e-30f) g.C[0] = sink;
    } else
    // a 256-column tile may reach past the last 128-column tile of N: nothing to store there, and the forward-only cross
    // entropy has no partial slot for it (a write would land in the next row's slots)
    if ((n0 + wn * 64) / 128 < (g.N + 127) / 128) {
        const EpiBias bias = epi_bias<EM>(g, z, n0 + wn * 64, lane);       // both halves have the same 64 columns: one load per tile
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {    // the wave's 128 x 64 tile as two 64 x 64 halves
            f32x16 (&sub)[2][2] = *reinterpret_cast<f32x16 (*)[2][2]>(&acc[2 * h2][0]);
            store_tile_at<EM>(g, sub, ep, z, m0 + wm * 128 + h2 * 64, n0 + wn * 64, (n0 + wn * 64) / 128, (g.N + 127) / 128, wn & 1, lane, bias);
        }
    }
    if (PROF && g.prof != nullptr && lane == 0) {
        __builtin_amdgcn_s_waitcnt(0);
        const unsigned long long p_end = __builtin_amdgcn_s_memtime();
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        unsigned long long* o = g.prof + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 8 + wave) * 8;
        o[0] = p_entry; o[1] = p_loop; o[2] = pacc[2]; o[3] = pacc[3]; o[4] = pacc[4]; o[5] = p_exit_loop; o[6] = p_end;
        o[7] = ((unsigned long long)xcc << 32) | hw;
    }
