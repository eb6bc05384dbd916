// fa_kv8_256_decode_loop.h -- the decode loop at head dim 256 over a cache of 8-bit floats (OCP e4m3fn, one byte per element), contiguous or
// paged, with or without a sliding window: the kernel of libflashattn_amd_kv8_256.so (fa_kv8_256_decode.hip instantiates it sixteen times).
// It is the 32-key block of fa_kv256_decode_loop.h with the data movement of fa_kv8_decode_body.h, re-budgeted; docs/kv_fp8_d256.md has the
// numbers.  No counterpart in the reference.
//
// Taken as they are: the workgroup (kv_tile), the share and empty-share handling, the Q fragments pinned in the accumulation half, the swapped
// product S^T = K Q^T on v_mfma_f32_32x32x16_bf16, kv256_mask_and_max / kv256_p_terms, the row sum against an all-ones operand, the page walk of
// two table entries per block fetched two blocks ahead (kv256_fetch_pages / kv256_pages_landed), the merge (kv_merge_and_store, SCALED).
//
// Arithmetic -- the contract of include/flashattn_amd_kv8.h.  e4m3 -> bf16 is exact, so K and V are dequantised WITHOUT their scales and meet
// the instruction sequence of fa_kv256_decode_loop.h: the same columns in the same matrix instruction in the same order.  k_scale arrives
// folded into the softmax scale, v_scale multiplies the normalised fp32 result once (here in an unsplit launch, in fa_kv8_combine.hip in a
// split one).  With v_scale a power of two the result is, bit for bit, v_scale x what fa_kv256_decode_loop.h gives on the dequantised cache.
//
// Data movement, per wave and 32-key block:
//   K  lane (lq, hi) loads 8 bytes at column 16 ks + 8 hi of key kv0 + lq, ks = 0 .. 15: 16 loads, 32 registers.  The bytes stay as they
//      came and pass through cvt_fp8x8 in front of the matrix instruction that takes them.
//   V  32 keys x 256 bytes = 8 KiB as eight 16-byte loads per lane (32 registers): load i is keys 4 i .. 4 i + 3, lane l holds the 16 columns
//      of column block l % 16 of key 4 i + l / 16 -- one 4-key group of the image per load, so a load never straddles a 16-row page group.
//      Converted (32 bytes of bf16) and stored with two ds_write_b128 into ONE 16 KiB bf16 image per wave, the [key/4][col/16][4][16]
//      sub-tiles of fa_bf16_common.h, which ds_read_b64_tr_b16 reads in the chunks of fa_kv256_decode_loop.h (four column blocks of O at a
//      time).  The image is written and read by the same wave inside one step, and a wave's LDS operations execute in order: no second
//      image, no barrier in the loop.
//   swizzle  a sub-tile is 128 bytes = eight 16-byte slots (key % 4, half).  The eight consecutive lanes one ds_write_b128 group serves hold
//      ONE key and eight consecutive column blocks cb, i.e. the SAME slot of eight sub-tiles 128 bytes apart: the same four banks eight
//      times.  The slot is XOR-ed with cb & 7: the eight lanes then take the eight different slots s ^ 0 .. s ^ 7, which tile 128 bytes, so
//      they fall on 32 distinct banks (and on distinct banks of a 64-bank LDS all the more).  cb & 7 takes every value once among any eight
//      consecutive column blocks, which is all the argument needs; 16 column blocks per row use each code twice, in different groups.  A
//      transposing read covers a whole sub-tile with 16 lanes, so a permutation inside sub-tiles leaves its banks as they were.
//   look-ahead  the raw bytes of block j + 1 (K and V: two register sets by name, the loop unrolled by two) are in flight while block j is
//      computed.  Every load is a register load, so the compiler counts vmcnt: 24 loads per block.
// Budgets: registers -- raw sets 2 x 64 (what the bf16 K sets took), Q 64 + O 128 + row sum 16 + scores 16 in the accumulation half, P 16 and
// the transient converted and V^T fragments in the other: one wave per SIMD at 512, no scratch.  LDS -- the merge's 33 280 bytes per wave is the
// larger term: 4 x 33 KiB + 1 KiB of (m, l) = 133 KiB.
// WINDOW adds the lower clamp max(., lo) on every K row, V row and table index and one select per score.  The clamp is what keeps a slid-out
// row out of the V image: there a NaN code would meet a zero weight in P.V and come out as NaN.
#pragma once
#include "fa_kv256_decode_loop.h"
#include "fa_kv8_256.h"
#include "fa_kv8_decode_core.h"

namespace fa {

struct Kv8x256Cfg {
    static constexpr int D = kKv256HeadDim, KS = D / 16, DB = D / 32;
    static constexpr int kBlk = Kv256Cfg::kBlk, kBlockPages = Kv256Cfg::kBlockPages, kVChunk = Kv256Cfg::kVChunk;
    static constexpr int LPR = D / 16;                        // lanes per V row: 16 bytes (16 columns) each
    static constexpr int kRowsPerLoad = kWave / LPR;          // keys one V load instruction covers: one 4-key group of the image
    static constexpr int kVLoads = kBlk / kRowsPerLoad;       // 16-byte V loads per lane and block
    static constexpr int kVImage = kBlk * 2 * D;              // bytes of the V image (32 keys, bf16)
    static constexpr int kGroupBytes = kRowsPerLoad * 2 * D;  // ... and of one 4-key group in it
    static constexpr int kLoadsPerBlock = KS + kVLoads;       // vector-memory instructions per lane and block
    static constexpr int kWaveLds = ((kVImage > Kv256Cfg::kMergeBytes ? kVImage : Kv256Cfg::kMergeBytes) + 1023) / 1024 * 1024;
    static_assert(kRowsPerLoad == 4 && kPagedMinPage % kRowsPerLoad == 0, "a V load is one key group and must not straddle a 16-row page group");
    static_assert(DB % kVChunk == 0 && kVChunk == 4, "the read offsets below are kept per column block modulo the chunk");
    static_assert(kKvWaves * kWaveLds + 2 * kKvWaves * kKvRowTile * 4 <= 160 * 1024, "the LDS of a CU");
};

// where a byte of the V image is kept: the 16-byte slot (bits 4 .. 6) XOR the low three bits of the sub-tile's column block
constexpr int v8x256_swz(int off) { return off ^ (((off >> 7) & 7) << 4); }

template <bool CAUSAL, bool OUT_F32, bool PAGED, bool WINDOW>
__device__ __forceinline__ void kv8_256_decode(const Kv8x256Params& wp)
{
    using C = Kv8x256Cfg;
    constexpr int D = C::D, KS = C::KS, DB = C::DB, BLK = C::kBlk, NP = C::kBlockPages, NV = C::kVLoads, LPR = C::LPR;
    __shared__ __attribute__((aligned(1024))) char smem[kKvWaves * C::kWaveLds];
    __shared__ float m_s[kKvWaves][kKvRowTile], l_s[kKvWaves][kKvRowTile];

    const PagedParams& pp = wp.k8.pg;
    const KvParams& p = pp.kv;
    int window_left = 0;
    if constexpr (WINDOW) window_left = wp.window_left;

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
    const int kbeg = tl.kbeg, kend = tl.kend;
    const int nblk = kend > kbeg ? (kend - kbeg + BLK - 1) / BLK : 0;   // 32-key blocks (tl.nblk counts 64-key ones)
    // WINDOW: the first key this lane's row sees, and the tile's (the lower clamp of every row that is loaded or looked up: kend > lo wherever
    // nblk > 0, since the tile's widest row reaches beyond its lowest key)
    int lo_row = 0;
    if constexpr (WINDOW) lo_row = tl.diag + (tl.row0 + lq) % p.nq - window_left;
    const int lo = tl.lo;

    bf16x8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = kv_q_fragment<D>(p.q, tl.prow0, row_ok, lq, hi, ks);
    // Q with O, the row sum and the scores in the accumulation half (224 of 256), the raw bytes' two sets, P and the transient fragments in
    // the other (fa_kv256_decode_loop.h): left to itself hipcc keeps Q where the raw bytes are and spills
    bf16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;
    auto q_in_acc_half = [&]() {   // ... and the all-ones operand with it: the raw bytes fill the other half to the last register
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+a"(qf[ks]));
        asm volatile("" : "+a"(ones));
    };
    q_in_acc_half();

    // one byte per element: every offset below is in bytes
    const uint8_t *kg, *vg;
    cst_i32_t* tbl = nullptr;
    int page_mask = 0;
    unsigned row_stride = 0;
    if constexpr (PAGED) {
        kg = (const uint8_t*)p.k + (int64_t)tl.head * pp.head_stride;
        vg = (const uint8_t*)p.v + (int64_t)tl.head * pp.head_stride;
        tbl = (cst_i32_t*)(pp.table + (int64_t)tl.seq * pp.max_pages);
        page_mask = (1 << pp.page_shift) - 1;
        row_stride = (unsigned)pp.row_stride;
    } else {
        kg = (const uint8_t*)p.k + (int64_t)tl.slab * p.kv_slab_stride;
        vg = (const uint8_t*)p.v + (int64_t)tl.slab * p.kv_slab_stride;
    }
    char* vbuf = smem + wave * C::kWaveLds;
    const int li = lane & 15, sub = (lane >> 4) & 1;
    // this lane's corner of a V^T fragment in the V image (keys permuted like the scores), per column block of a chunk: the swizzle depends on
    // the sub-tile's column block 2 db + sub modulo 8 alone, i.e. on db % 4
    // this lane's corner of a V^T fragment in the V image (keys permuted like the scores), for column block 0.  The swizzle depends on the
    // sub-tile's column block 2 db + sub modulo 8 alone: column block d0 + i of a chunk is at (v_rd ^ (i << 5)) + 2 (d0 + i) sub-tiles
    int v_rd = v8x256_swz((hi * LPR + sub) * 128 + (li >> 2) * 32 + (li & 3) * 8);
    // ... and where this lane's 16 columns of a V load go inside the load's key group: key lane / 16, column block lane % 16, as two
    // 16-byte halves at v_wr and v_wr ^ 16
    int v_wr = v8x256_swz((lane % LPR) * 128 + (lane / LPR) * 32);
    static_assert(v8x256_swz(2 * 128) == (2 * 128 ^ 32) && v8x256_swz(128 + 16) == 128, "what the two XORs above rely on");
    const float c = p.scale_log2e;

    f32x16 o[DB], lacc;
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) lacc[r] = 0.0f;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] = 0.0f;

    // the row of the cache that key `key` loads: itself inside [lo, kend), the nearest row of that range outside
    auto row_of = [&](int key) {
        int row = min(key, kend - 1);
        if constexpr (WINDOW) row = max(row, lo);
        return row;
    };
    // The bytes of the block that starts at key kv0: K as KS 8-byte pieces of key kv0 + lq, V as NV 16-byte pieces.  pb: its page offsets.
    // Addresses are a uniform 64-bit base plus a 32-bit byte offset per lane (a slab stays below 2^32 bytes, and so does the offset inside a
    // page: the host checks both).
    // The lane's coordinates are derived from its number HERE, behind an empty statement, not held through the loop (hipcc would hoist
    // them): five registers less where the budget is met to the last one.
    int lane_v = lane;
    auto load_block = [&](int kv0, const int64_t(&pb)[NP], u32x2(&kf)[KS], u32x4(&vf)[NV]) {
        asm volatile("" : "+v"(lane_v));
        const int lq = lane_v & 31, hi = lane_v >> 5, v_key = lane_v / LPR, v_cb = lane_v % LPR;
        const int krow = row_of(kv0 + lq);
        const uint8_t* kr;
        if constexpr (PAGED)   // (a select between the two array elements themselves becomes an indexed read of the array: scratch)
            kr = kg + pb[0] + ((lq & 16) ? pb[1] - pb[0] : (int64_t)0) + ((unsigned)(krow & page_mask) * row_stride + hi * 8);
        else
            kr = kg + ((unsigned)krow * (unsigned)D + hi * 8);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[ks] = *(const u32x2*)(kr + ks * 16);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int row = row_of(kv0 + i * C::kRowsPerLoad + v_key);
            const uint8_t* vr;
            if constexpr (PAGED)   // the 16-key group of a piece is the same in every lane
                vr = vg + pb[i * C::kRowsPerLoad / kPagedMinPage] + ((unsigned)(row & page_mask) * row_stride + v_cb * 16);
            else
                vr = vg + ((unsigned)row * (unsigned)D + v_cb * 16);
            vf[i] = *(const u32x4*)vr;
        }
    };

    // One block.  The raw bytes ping-pong between two register sets by NAME (the loop below is unrolled by two): a copy "current = next" at
    // the end of a step would have to wait for the next block's loads.
    // PAGED: the table runs two blocks ahead of the loads: pg[] holds the page offsets of the block whose loads the next step issues, ent[] the
    // entries of the block after that, in flight from the end of one step to the end of the next.
    int64_t pg[NP];
    int ent[NP];
    auto step = [&](int blk, const u32x2(&kcur)[KS], const u32x4(&vcur)[NV], u32x2(&knext)[KS], u32x4(&vnext)[NV]) __attribute__((always_inline)) {
        const int kv0 = kbeg + blk * BLK;
        // The wave's next block, unconditionally.  Past the share's end every lane's row is redirected to the share's last row (one cached
        // row per load), so the last step costs no traffic and the loop body has no branch.
        load_block(kv0 + kKvWaves * BLK, pg, knext, vnext);
        // The loads stay HERE: their values are first used in the next step, which for every second step sits behind the loop's `if`, and
        // without this statement the compiler sinks them down to that use -- nothing would be in flight while this block is computed.
        asm volatile("" ::: "memory");

        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            u32x2 kk = kcur[ks];
            asm volatile("" : "+v"(kk));   // ... and this block's products stay BEHIND them: hoisted above, they would be waited for with nothing new in flight
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cvt_fp8x8(kk[0], kk[1]), qf[ks], s, 0, 0, 0);
        }

        // this block's V: bf16 into the image (the previous step's reads of it were issued before these stores: LDS runs in order)
        // The lane's addresses in the image are derived where they are used, from ONE register each for the stores and for the reads: held
        // through the loop they are six, and the arithmetic half has none to spare (the empty statements keep hipcc from hoisting them)
        asm volatile("" : "+v"(v_wr));
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            char* dst = vbuf + i * C::kGroupBytes;
            *(bf16x8*)(dst + v_wr) = cvt_fp8x8(vcur[i][0], vcur[i][1]);
            *(bf16x8*)(dst + (v_wr ^ 16)) = cvt_fp8x8(vcur[i][2], vcur[i][3]);
        }

        bf16x8 ph[2], pl[2];
        const KvRescale rs = kv256_mask_and_max<WINDOW>(s, lim - kv0 - 4 * hi, c, m, lo_row - kv0 - 4 * hi);
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] *= rs.alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) lacc[r] *= rs.alpha;
        kv256_p_terms(s, rs.m_use, ph, pl);

#pragma unroll
        for (int t = 0; t < 2; ++t) {   // 16 keys: key groups 4 t + hi and 4 t + 2 + hi
#pragma unroll
            for (int d0 = 0; d0 < DB; d0 += C::kVChunk) {   // kVChunk column blocks of O at a time: the fragments in flight stay few
                s16x4 vv[2 * C::kVChunk];
                asm volatile("" : "+v"(v_rd));
#pragma unroll
                for (int i = 0; i < C::kVChunk; ++i) {
                    const char* src = vbuf + (v_rd ^ (i << 5)) + (4 * t * LPR + 2 * (d0 + i)) * 128;
                    vv[2 * i] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)src);
                    vv[2 * i + 1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(src + 2 * LPR * 128));
                }
#pragma unroll
                for (int i = 0; i < C::kVChunk; ++i) {
                    const bf16x8 vf = __builtin_bit_cast(bf16x8, __builtin_shufflevector(vv[2 * i], vv[2 * i + 1], 0, 1, 2, 3, 4, 5, 6, 7));
                    o[d0 + i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, ph[t], o[d0 + i], 0, 0, 0);
                    o[d0 + i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pl[t], o[d0 + i], 0, 0, 0);
                }
            }
            lacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, ph[t], lacc, 0, 0, 0);
            lacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, pl[t], lacc, 0, 0, 0);
        }
        if constexpr (PAGED) {
            // The step's matrix instructions are issued before the table is touched: lgkmcnt counts scalar loads and LDS reads together, so a
            // product scheduled behind the fetch below would wait for a table round trip together with its V^T fragment (docs/kv_fp8.md)
#pragma unroll
            for (int db = 0; db < DB; ++db) asm volatile("" : "+a"(o[db]));
            asm volatile("" : "+a"(lacc));
            kv256_pages_landed(ent, pp.page_stride, pg);                                                // the block the next step issues: fetched a step ago
            kv256_fetch_pages<WINDOW>(tbl, pp.page_shift, kv0 + 3 * kKvWaves * BLK, kend, ent, lo);     // the block after that
        }
        q_in_acc_half();
    };

    u32x2 ka[KS], kb[KS];
    u32x4 va[NV], vb[NV];
#pragma unroll
    for (int i = 0; i < NP; ++i) pg[i] = 0, ent[i] = 0;
    if (wave < nblk) {   // kend >= 1 from here on: every row (and, PAGED, every table index) is that of a key below len
        if constexpr (PAGED) {
            int e0[NP], e1[NP];
            kv256_fetch_pages<WINDOW>(tbl, pp.page_shift, kbeg + wave * BLK, kend, e0, lo);
            kv256_fetch_pages<WINDOW>(tbl, pp.page_shift, kbeg + (wave + kKvWaves) * BLK, kend, e1, lo);
            int64_t p0[NP];
            kv256_pages_landed(e0, pp.page_stride, p0);
            load_block(kbeg + wave * BLK, p0, ka, va);
            kv256_pages_landed(e1, pp.page_stride, pg);
            kv256_fetch_pages<WINDOW>(tbl, pp.page_shift, kbeg + (wave + 2 * kKvWaves) * BLK, kend, ent, lo);
        } else {
            load_block(kbeg + wave * BLK, pg, ka, va);
        }
    }
    asm volatile("" ::: "memory");
    for (int blk = wave; blk < nblk; blk += 2 * kKvWaves) {
        step(blk, ka, va, kb, vb);
        if (blk + kKvWaves < nblk) step(blk + kKvWaves, kb, vb, ka, va);
    }

    mfma_drain();   // the loop exit is a branch: the last matrix instructions may still be in flight; the image's last reads have been consumed
    kv_merge_and_store<D, OUT_F32, true, C::kWaveLds>(p, tl, smem, m_s, l_s, wave, lq, hi, m, o, lacc, wp.k8.v_scale);
}

}  // namespace fa
