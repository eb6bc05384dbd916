// fa_kv_decode16_body.h -- the decode loop over a 16-bit (bf16) cache, contiguous (fa_kv_decode.hip) or paged (fa_paged_decode.hip): ONE body,
// included as text INSIDE the two kernels.  fa_kv_decode_core.h has the workgroup, the arithmetic, the merge and the page walk.
//
// Why text and not a function: reached through one more level of inlining, hipcc gives the d = 64 paged loop another register assignment
// (the K register sets as eight vectors instead of one, one wait less in the prologue, 36 instructions fewer) -- harmless, but
// tests/test_kv_code_profile.py holds every kernel to its recorded instruction profile, and as text in the kernel the body compiles to it.
//
// The including kernel provides, in namespace fa, with fa_kv_decode_core.h included:
//   D, CAUSAL, OUT_F32      its template parameters
//   PAGED, P_TERMS          constexpr bool / int
//   WINDOW, window_left     constexpr bool; an int (named only behind `if constexpr (WINDOW)` and as kv_tile's ignored argument otherwise)
//   p                       const KvParams&
//   pp                      const PagedParams& where PAGED; any PagedParams otherwise (it is named only behind `if constexpr (PAGED)`)
//
// Data movement, per wave and 64-key block:
//   K  straight to registers: the A operand of K Q^T is "lane (key, half) holds 8 consecutive columns of its key", i.e. one 16-byte
//      load per lane and 16 columns -- an operand streamed once gains nothing from an LDS round trip
//   V  the second product contracts over keys and needs V^T fragments; those come from ds_read_b64_tr_b16 over the V image of
//      fa_bf16_common.h, which LDS-DMA (16 bytes per lane, no register staging) fills.  Two images per wave: block j + 1 (K registers
//      and V image) is in flight while block j is computed -- 4 waves x 32 KiB at d = 128, and the buffers are private to a wave, so
//      the loop has no barrier.
// PAGED differs in how a row's address is formed, and in nothing else: the results are the same bits on the gathered cache.
// WINDOW (fa_kvw_decode.hip) differs in where the tile's shares start (kv_tile), in one more select per score (kv_mask_and_max) and in a
// lower clamp max(., lo) beside the upper one on every K row, V row and table index: no load, product, exponential or LDS byte more.
    constexpr int NP = kPagedBlockPages;
    using C = KvCfg<D>;
    constexpr int KS = C::KS, DB = C::DB;
    __shared__ __attribute__((aligned(1024))) char smem[kKvWaves * C::kWaveLds];
    __shared__ float m_s[kKvWaves][kKvRowTile], l_s[kKvWaves][kKvRowTile];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lq = lane & 31, hi = lane >> 5;

    int heads_kv = 1;
    if constexpr (PAGED) heads_kv = pp.heads_kv;
    const KvTile tl = kv_tile<CAUSAL, WINDOW>(p, heads_kv, window_left);
    if (kv_share_is_empty(p, tl)) {
        kv_mark_share_empty(p, tl);
        return;
    }
    const bool row_ok = kv_row_ok(p, tl, lq);
    const int lim = kv_last_visible_key<CAUSAL>(p, tl, lq);
    const int slab = tl.slab, seq = tl.seq, head = tl.head, kbeg = tl.kbeg, kend = tl.kend, nblk = tl.nblk;
    // WINDOW: the first key this lane's row sees, and the tile's (the lower clamp of every row that is loaded or looked up: kend > lo
    // wherever nblk > 0, since the tile's widest row reaches beyond its lowest key)
    int lo_row = 0;
    if constexpr (WINDOW) lo_row = tl.diag + (tl.row0 + lq) % p.nq - window_left;
    const int lo = tl.lo;

    bf16x8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = kv_q_fragment<D>(p.q, tl.prow0, row_ok, lq, hi, ks);
    bf16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;

    const __bf16 *kg, *vg;
    cst_i32_t* tbl = nullptr;
    int page_mask = 0;
    unsigned row_stride = 0;
    if constexpr (PAGED) {
        kg = (const __bf16*)p.k + (int64_t)head * pp.head_stride;
        vg = (const __bf16*)p.v + (int64_t)head * pp.head_stride;
        tbl = (cst_i32_t*)(pp.table + (int64_t)seq * pp.max_pages);
        page_mask = (1 << pp.page_shift) - 1;
        row_stride = (unsigned)pp.row_stride;
    } else {
        kg = (const __bf16*)p.k + (int64_t)slab * p.kv_slab_stride;
        vg = (const __bf16*)p.v + (int64_t)slab * p.kv_slab_stride;
    }
    char* vbuf = smem + wave * C::kWaveLds;
    const int li = lane & 15;
    // this lane's corner of a V^T fragment in the V image (fa_bf16_common.h: [key/4][col/16][4][16] sub-tiles, keys permuted like the scores)
    const int v_lane_off = (hi * (D / 16) + ((lane >> 4) & 1)) * 128 + (li >> 2) * 32 + (li & 3) * 8;
    const float c = p.scale_log2e;

    f32x16 o[DB], lacc;
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) lacc[r] = 0.0f;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] = 0.0f;

    bf16x8 kc[2][KS], kn[2][KS];
    // the K fragments and the V image of the block that starts at key kv0; pb: its page offsets (PAGED)
    auto load_k = [&](int kv0, const int64_t(&pb)[NP], bf16x8(&kf)[2][KS]) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            int row = min(kv0 + kb * 32 + lq, kend - 1);
            if constexpr (WINDOW) row = max(row, lo);
            const __bf16* kr;
            if constexpr (PAGED)
                kr = kg + page_of_k_row(pb, kb, lq) + (unsigned)(row & page_mask) * row_stride + hi * 8;
            else
                kr = kg + (int64_t)row * D + hi * 8;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) kf[kb][ks] = *(const bf16x8*)(kr + ks * 16);
        }
    };
    auto issue_v = [&](int kv0, const int64_t(&pb)[NP], char* dst) {
        if constexpr (PAGED) {   // issue_v_tile (fa_bf16_common.h) for one wave, through the pages: the 16-key group of a piece is the same in every lane
#pragma unroll
            for (int ch = 0; ch < C::kVTile / 1024; ++ch) {
                const int blk = ch * 8 + lane / 8;
                const int kg4 = blk / (D / 16), cb = blk % (D / 16);
                const int key = kg4 * 4 + (lane % 8) / 2;
                const int col = cb * 16 + (lane & 1) * 8;
                constexpr int kKeysPerPiece = 512 / D;   // a 1 KiB piece holds whole rows of 2 D bytes
                static_assert(kPagedMinPage % kKeysPerPiece == 0, "a piece must not straddle a 16-key group");
                int row = min(kv0 + key, kend - 1);
                if constexpr (WINDOW) row = max(row, lo);
                const __bf16* src = vg + pb[ch * kKeysPerPiece / kPagedMinPage] + (unsigned)(row & page_mask) * row_stride + col;
                __builtin_amdgcn_global_load_lds((gbl_cvoid_t*)src, (lds_void_t*)(dst + ch * 1024), 16, 0, 0);
            }
        } else if constexpr (WINDOW) {
            issue_v_tile_from<D>(vg, kv0, lo, kend, dst, lane);
        } else {
            issue_v_tile<D, 1>(vg, kv0, kend, D, dst, 0, lane);
        }
    };

    // One block.  The K fragments ping-pong between two register sets by NAME (the loop below is unrolled by two): a copy "current = next" at
    // the end of a step would have to wait for the next block's loads.
    // PAGED: the table runs two blocks ahead of the loads: pg[] holds the page offsets of the block whose loads the next step issues, ent[] the
    // entries of the block after that, in flight from the end of one step to the end of the next.
    int64_t pg[NP];
    int ent[NP];
    auto step = [&](int blk, int par, const bf16x8(&kcur)[2][KS], bf16x8(&knext)[2][KS]) __attribute__((always_inline)) {
        const int kv0 = kbeg + blk * kKvBlk;
        // The wave's next block, unconditionally: K to the spare registers, V to the other image.  Past the share's end every lane's row is
        // redirected to the share's last row (one cached row per load), so the last step costs no traffic, the loop body has no branch, and
        // the number of loads in flight is the same in every step -- which is what lets the waits below count.
        load_k(kv0 + kKvWaves * kKvBlk, pg, knext);
        issue_v(kv0 + kKvWaves * kKvBlk, pg, vbuf + (par ^ 1) * C::kVTile);

        f32x16 s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kb][r] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kcur[kb][ks], qf[ks], s[kb], 0, 0, 0);

        bf16x8 ph[4], pl[4];
        const KvRescale rs = kv_mask_and_max<WINDOW>(s, lim - kv0 - 4 * hi, c, m, lo_row - kv0 - 4 * hi);
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] *= rs.alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) lacc[r] *= rs.alpha;
        kv_p_terms(s, rs.m_use, ph, pl);

        // this block's V image has landed once only the next block's loads are outstanding
        wait_vm_outstanding<C::kLoadsPerBlock>();
        const unsigned v_addr = (unsigned)(size_t)(lds_void_t*)(vbuf + par * C::kVTile + v_lane_off);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int f = kb * 2 + t;
                s16x4 vv[2 * DB];
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    vv[2 * db] = lds_read_tr16(v_addr + ((kb * 8 + 4 * t + 0) * (D / 16) + 2 * db) * 128);
                    vv[2 * db + 1] = lds_read_tr16(v_addr + ((kb * 8 + 4 * t + 2) * (D / 16) + 2 * db) * 128);
                }
                lds_reads_landed(vv);
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    const bf16x8 vf = __builtin_bit_cast(bf16x8, __builtin_shufflevector(vv[2 * db], vv[2 * db + 1], 0, 1, 2, 3, 4, 5, 6, 7));
                    o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, ph[f], o[db], 0, 0, 0);
                    if (P_TERMS == 2) o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pl[f], o[db], 0, 0, 0);
                }
                lacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, ph[f], lacc, 0, 0, 0);
                if (P_TERMS == 2) lacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, pl[f], lacc, 0, 0, 0);
            }
        if constexpr (PAGED) {
            pages_landed(ent, pp.page_stride, pg);                                        // the block the next step issues: fetched a step ago
            fetch_pages<WINDOW>(tbl, pp.page_shift, kv0 + 3 * kKvWaves * kKvBlk, kend, ent, lo);   // the block after that
        }
        asm volatile("" ::: "memory");   // the image is read before the next step's DMA may be enqueued over its twin
    };

#pragma unroll
    for (int i = 0; i < NP; ++i) pg[i] = 0, ent[i] = 0;
    if (wave < nblk) {   // kend >= 1 from here on: every row (and, PAGED, every table index) is that of a key below len
        if constexpr (PAGED) {
            int e0[NP], e1[NP];
            fetch_pages<WINDOW>(tbl, pp.page_shift, kbeg + wave * kKvBlk, kend, e0, lo);
            fetch_pages<WINDOW>(tbl, pp.page_shift, kbeg + (wave + kKvWaves) * kKvBlk, kend, e1, lo);
            int64_t p0[NP];
            pages_landed(e0, pp.page_stride, p0);
            load_k(kbeg + wave * kKvBlk, p0, kc);
            issue_v(kbeg + wave * kKvBlk, p0, vbuf);
            pages_landed(e1, pp.page_stride, pg);
            fetch_pages<WINDOW>(tbl, pp.page_shift, kbeg + (wave + 2 * kKvWaves) * kKvBlk, kend, ent, lo);
        } else {
            load_k(kbeg + wave * kKvBlk, pg, kc);
            issue_v(kbeg + wave * kKvBlk, pg, vbuf);
        }
    }
    asm volatile("" ::: "memory");
    for (int blk = wave; blk < nblk; blk += 2 * kKvWaves) {
        step(blk, 0, kc, kn);
        if (blk + kKvWaves < nblk) step(blk + kKvWaves, 1, kn, kc);
    }

    mfma_drain();     // the loop exit is a branch: the last matrix instructions may still be in flight
    wait_lds_dma();   // the last step's look-ahead still targets an image; after it the merge may take the wave's V images
    // hipcc cannot see that wait (it is inline asm) and adds one of its own where the merge first overwrites a register the look-ahead K loads
    // target -- at the top of the merge, or inside its `hi == 0` branch and again behind it, as the register allocation falls.  The d = 128
    // kernels of the unwindowed libraries have the one at the top; a wait hipcc can see puts the windowed ones' there whatever the allocation is.
    if constexpr (WINDOW && D == 128) {
        __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0) alone
        __builtin_amdgcn_sched_barrier(0);    // ... and nothing of the merge is scheduled in front of it
    }
    kv_merge_and_store<D, OUT_F32, false, C::kWaveLds>(p, tl, smem, m_s, l_s, wave, lq, hi, m, o, lacc, 1.0f);
