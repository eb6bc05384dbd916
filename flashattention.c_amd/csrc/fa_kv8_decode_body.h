// fa_kv8_decode_body.h -- the decode loop over a cache of 8-bit floats (OCP e4m3fn, one byte per element), contiguous or paged: ONE body,
// included as text INSIDE the kernels of fa_kv8_decode.hip (WINDOW = false) and fa_kvw8_decode.hip (WINDOW = true), the way
// fa_kv_decode16_body.h is the loop of the 16-bit kernels.  fa_kv_decode_core.h has the workgroup, the arithmetic, the merge and the page
// walk; fa_kv8_decode_core.h the block geometry, the conversion and the swizzle.  No counterpart in the reference.
//
// The including kernel provides, in namespace fa, with fa_kv8_decode_core.h included:
//   D, CAUSAL, OUT_F32, PAGED   its template parameters
//   WINDOW, window_left         constexpr bool; an int (named only behind `if constexpr (WINDOW)` and as kv_tile's ignored argument otherwise)
//   pp, p                       const PagedParams&, const KvParams& (a contiguous cache: pp.kv alone, the paged fields unused)
//   v_scale                     float
//
// Arithmetic -- the contract of include/flashattn_amd_kv8.h.  e4m3 -> bf16 is exact for every non-NaN code, so K and V are dequantised to
// bf16 WITHOUT their scales and then meet the very instruction sequence of the 16-bit kernels.  k_scale arrives folded into the softmax scale
// (host, one fp32 product); v_scale multiplies the normalised fp32 result once: here, before the store to o, in an unsplit launch; in
// fa_kv8_combine.hip, behind the merge of the shares, in a split one.  With v_scale a power of two the result is, bit for bit, v_scale x what
// the 16-bit kernels give on the cache dequantised to bf16.
//
// Data movement, per wave and 64-key block -- what differs from fa_kv_decode16_body.h:
//   K  the A operand of K Q^T is "lane (key, half) holds 8 consecutive columns of its key per 16-column step": one 8-byte load at
//      ks * 16 + hi * 8 (the 16-bit kernels: one 16-byte load).  The bytes stay in registers as they came and are converted
//      (v_cvt_pk_f32_fp8, then the pack to bf16) in front of the matrix instruction that takes them.
//   V  the second product contracts over keys and needs V^T fragments.  A lane loads 16 bytes = 16 columns of one key, converts them to
//      32 bytes of bf16 and stores those into the V image of fa_bf16_common.h ([key/4][col/16][4][16] sub-tiles), which ds_read_b64_tr_b16
//      reads as before.  Inside a 128-byte sub-tile the 16-byte slots are XOR-ed with the sub-tile's column block (v_swz): the eight
//      consecutive lanes one ds_write_b128 group serves hold one or two keys across the column blocks, which would all fall on the same
//      banks; a transposing read covers whole sub-tiles and stays conflict-free under any permutation inside them.
// Every load is a register load: the compiler counts vmcnt itself.  The look-ahead is kept -- the bytes of block j + 1 (K and V, registers)
// are in flight while block j is computed -- and the image is written and read by the same wave inside one step (LDS operations of a wave
// execute in order), so one image per wave suffices: half the LDS of the 16-bit kernels and no barrier in the loop.
//
// WINDOW (include/flashattn_amd_kvw8.h) differs in where the tile's shares start (kv_tile), in one more select per score and in a lower
// clamp max(., lo) beside the upper one on every K row, V row and table index: no load, product, exponential, barrier or LDS access more.
// The clamp is what keeps a slid-out row out of the V image: there a NaN code would meet a zero weight in P.V and come out as NaN.
    constexpr int NP = kPagedBlockPages;
    using C = Kv8Cfg<D>;
    constexpr int KS = C::KS, DB = C::DB, LPR = C::LPR, NV = C::kVLoads;
    __shared__ __attribute__((aligned(1024))) char smem[kKvWaves * C::kWaveLds];
    __shared__ float m_s[kKvWaves][kKvRowTile], l_s[kKvWaves][kKvRowTile];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lq = lane & 31, hi = lane >> 5;

    const KvTile tl = kv_tile<CAUSAL, WINDOW>(p, PAGED ? pp.heads_kv : 1, window_left);
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

    // one byte per element: every offset below is in bytes
    const uint8_t* kg = (const uint8_t*)p.k + (PAGED ? (int64_t)head * pp.head_stride : (int64_t)slab * p.kv_slab_stride);
    const uint8_t* vg = (const uint8_t*)p.v + (PAGED ? (int64_t)head * pp.head_stride : (int64_t)slab * p.kv_slab_stride);
    cst_i32_t* tbl = (cst_i32_t*)(pp.table + (int64_t)seq * pp.max_pages);
    const int page_mask = (1 << pp.page_shift) - 1;
    const unsigned row_stride = (unsigned)pp.row_stride;
    char* vbuf = smem + wave * C::kWaveLds;
    const int li = lane & 15;
    // this lane's corner of a V^T fragment in the V image, per 32-column block (the swizzle depends on the column block, not on the key group)
    int v_rd_off[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db)
        v_rd_off[db] = v_swz<D>((hi * (D / 16) + ((lane >> 4) & 1) + 2 * db) * 128 + (li >> 2) * 32 + (li & 3) * 8);
    // ... and where this lane's 16 columns of a V load go: key lane / LPR of the load's rows, column block lane % LPR, as two 16-byte halves
    const int v_key = lane / LPR, v_cb = lane % LPR;
    const int v_wr_lo = v_swz<D>(((v_key / 4) * LPR + v_cb) * 128 + (v_key % 4) * 32);
    const int v_wr_hi = v_swz<D>(((v_key / 4) * LPR + v_cb) * 128 + (v_key % 4) * 32 + 16);
    const float c = p.scale_log2e;

    f32x16 o[DB], lacc;
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) lacc[r] = 0.0f;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] = 0.0f;

    // The bytes of one block: K as KS 8-byte pieces for each of the lane's two keys, V as NV 16-byte pieces.  pb: its page offsets (PAGED)
    auto load_block = [&](int kv0, const int64_t(&pb)[NP], u32x2(&kf)[2][KS], u32x4(&vf)[NV]) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            int row = min(kv0 + kb * 32 + lq, kend - 1);
            if constexpr (WINDOW) row = max(row, lo);
            const uint8_t* kr;
            if constexpr (PAGED)
                kr = kg + page_of_k_row(pb, kb, lq) + (unsigned)(row & page_mask) * row_stride + hi * 8;
            else
                kr = kg + (int64_t)row * D + hi * 8;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) kf[kb][ks] = *(const u32x2*)(kr + ks * 16);
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            int row = min(kv0 + i * C::kRowsPerLoad + v_key, kend - 1);
            if constexpr (WINDOW) row = max(row, lo);
            const uint8_t* vr;
            if constexpr (PAGED)   // the 16-key group of a piece is the same in every lane
                vr = vg + pb[i * C::kRowsPerLoad / kPagedMinPage] + (unsigned)(row & page_mask) * row_stride + v_cb * 16;
            else
                vr = vg + (int64_t)row * D + v_cb * 16;
            vf[i] = *(const u32x4*)vr;
        }
    };

    // One block.  The K and V bytes ping-pong between two register sets by NAME (the loop below is unrolled by two): a copy "current = next"
    // at the end of a step would have to wait for the next block's loads.
    // PAGED: the table runs two blocks ahead of the loads: pg[] holds the page offsets of the block whose loads the next step issues, ent[]
    // the entries of the block after that, in flight from the end of one step to the end of the next.
    int64_t pg[NP];
    int ent[NP];
    auto step = [&](int blk, const u32x2(&kcur)[2][KS], const u32x4(&vcur)[NV], u32x2(&knext)[2][KS], u32x4(&vnext)[NV]) __attribute__((always_inline)) {
        const int kv0 = kbeg + blk * kKvBlk;
        // The wave's next block, unconditionally.  Past the share's end every lane's row is redirected to the share's last row (one cached
        // row per load), so the last step costs no traffic and the loop body has no branch.
        load_block(kv0 + kKvWaves * kKvBlk, pg, knext, vnext);
        // The loads stay HERE: their values are first used in the next step, which for every second step sits behind the loop's `if`, and
        // without this statement the compiler sinks them down to that use -- nothing would be in flight while this block is computed.
        asm volatile("" ::: "memory");

        f32x16 s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kb][r] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                u32x2 kk = kcur[kb][ks];
                asm volatile("" : "+v"(kk));   // ... and this block's products stay BEHIND them: hoisted above, they would be waited for with nothing new in flight
                s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cvt_fp8x8(kk[0], kk[1]), qf[ks], s[kb], 0, 0, 0);
            }

        // this block's V: bf16 into the image (the previous step's reads of it were issued before these stores: LDS runs in order)
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            char* dst = vbuf + i * (kWave * 32);   // kRowsPerLoad keys = kRowsPerLoad / 4 key groups of LPR sub-tiles: 2 KiB per load
            *(bf16x8*)(dst + v_wr_lo) = cvt_fp8x8(vcur[i][0], vcur[i][1]);
            *(bf16x8*)(dst + v_wr_hi) = cvt_fp8x8(vcur[i][2], vcur[i][3]);
        }

        bf16x8 ph[4], pl[4];
        // kv_mask_and_max (fa_kv_decode_core.h) written out: called as a function here, hipcc moves four of the sixteen unwindowed kernels off
        // their recorded instruction profile (two VGPRs more, other vmcnt waits), and tests/test_kv_code_profile.py holds them to it
        const int rel = lim - kv0 - 4 * hi;   // key offset (kb * 32 + (r & 3) + 8 * (r >> 2)) > rel: not visible
        int rel_lo = 0;                       // WINDOW: neither is a key offset < rel_lo
        if constexpr (WINDOW) rel_lo = lo_row - kv0 - 4 * hi;
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float t = (kb * 32 + (r & 3) + 8 * (r >> 2) > rel) ? -INFINITY : s[kb][r] * c;
                if constexpr (WINDOW) t = (kb * 32 + (r & 3) + 8 * (r >> 2) < rel_lo) ? -INFINITY : t;
                s[kb][r] = t;
                mx = fmaxf(mx, t);
            }
        mx = xhalf_max(mx);
        const float m_new = fmaxf(m, mx);
        const float m_use = (m_new == -INFINITY) ? 0.0f : m_new;   // a row that has seen no key yet: p = 0, no NaN
        const float alpha = fast_exp2(m - m_use);
        m = m_new;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) lacc[r] *= alpha;
        kv_p_terms(s, m_use, ph, pl);

#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int f = kb * 2 + t;
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    const char* src = vbuf + v_rd_off[db];
                    const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(src + (kb * 8 + 4 * t + 0) * (D / 16) * 128));
                    const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(src + (kb * 8 + 4 * t + 2) * (D / 16) * 128));
                    const bf16x8 vf = __builtin_bit_cast(bf16x8, __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
                    o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, ph[f], o[db], 0, 0, 0);
                    o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pl[f], o[db], 0, 0, 0);
                }
                lacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, ph[f], lacc, 0, 0, 0);
                lacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, pl[f], lacc, 0, 0, 0);
            }
        if constexpr (PAGED) {
            // The step's matrix instructions are issued before the table is touched: lgkmcnt counts scalar loads and LDS reads together, so a
            // product scheduled behind the fetch below would wait for a table round trip together with its V^T fragment (measured with pages
            // of 16 rows, where every step touches a new line of the table: 1.26-1.29 x the contiguous cache before this, docs/kv_fp8.md).
#pragma unroll
            for (int db = 0; db < DB; ++db) asm volatile("" : "+v"(o[db]));
            asm volatile("" : "+v"(lacc));
            pages_landed(ent, pp.page_stride, pg);                                                 // the block the next step issues: fetched a step ago
            fetch_pages<WINDOW>(tbl, pp.page_shift, kv0 + 3 * kKvWaves * kKvBlk, kend, ent, lo);   // the block after that
        }
    };

    u32x2 ka[2][KS], kb_[2][KS];
    u32x4 va[NV], vb[NV];
#pragma unroll
    for (int i = 0; i < NP; ++i) pg[i] = 0, ent[i] = 0;
    if (wave < nblk) {   // kend >= 1 from here on: every row (and, PAGED, every table index) is that of a key below len
        if constexpr (PAGED) {
            int e0[NP], e1[NP];
            fetch_pages<WINDOW>(tbl, pp.page_shift, kbeg + wave * kKvBlk, kend, e0, lo);
            fetch_pages<WINDOW>(tbl, pp.page_shift, kbeg + (wave + kKvWaves) * kKvBlk, kend, e1, lo);
            int64_t p0[NP];
            pages_landed(e0, pp.page_stride, p0);
            load_block(kbeg + wave * kKvBlk, p0, ka, va);
            pages_landed(e1, pp.page_stride, pg);
            fetch_pages<WINDOW>(tbl, pp.page_shift, kbeg + (wave + 2 * kKvWaves) * kKvBlk, kend, ent, lo);
        } else {
            load_block(kbeg + wave * kKvBlk, pg, ka, va);
        }
    }
    for (int blk = wave; blk < nblk; blk += 2 * kKvWaves) {
        step(blk, ka, va, kb_, vb);
        if (blk + kKvWaves < nblk) step(blk + kKvWaves, kb_, vb, ka, va);
    }

    mfma_drain();   // the loop exit is a branch: the last matrix instructions may still be in flight; the image's last reads have been consumed
    kv_merge_and_store<D, OUT_F32, true, C::kWaveLds>(p, tl, smem, m_s, l_s, wave, lq, hi, m, o, lacc, v_scale);
