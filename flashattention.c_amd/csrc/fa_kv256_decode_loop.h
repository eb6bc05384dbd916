// fa_kv256_decode_loop.h -- the decode loop at head dim 256 over a bf16 cache, contiguous or paged, with or without a sliding window: the
// kernel of libflashattn_amd_kv256.so (fa_kv256_decode.hip instantiates it sixteen times).  fa_kv_decode_core.h has the workgroup (kv_tile),
// the arithmetic contract, the merge and the conventions of the page walk; they are used here as they are.
//
// What is the same as in fa_kv_decode16_body.h: a workgroup owns (K/V slab, 32-row tile of packed rows, key share); the swapped product
// S^T = K Q^T on v_mfma_f32_32x32x16_bf16, so a lane holds the scores of ONE row; one bf16 product for Q.K^T, P as bf16 hi + bf16 lo, the row
// sum on the matrix pipe against an all-ones operand in the instruction sequence of every O column; four waves with an online-softmax state
// each, merged through LDS; loads of rows outside [lo, kend) redirected to the nearest row inside; no barrier in the loop.
//
// What differs is the block: 32 keys, not 64.  Wave w walks blocks w, w + 4, ... of 32 keys of the share (shares start at multiples of 64,
// so blocks start at multiples of 32).  Per wave and block:
//   K  straight to registers: ONE 32-key MFMA row block, KS = 16 loads of 16 bytes per lane; two register sets by name (2 x 64 VGPRs)
//   V  LDS-DMA into a 16 KiB image (32 keys x 512 bytes, the [key/4][col/16][4][16] sub-tiles of fa_bf16_common.h), read with
//      ds_read_b64_tr_b16; two images per wave, so block j + 1 is in flight while block j is computed
// The budgets a 64-key block breaks and this one keeps:
//   LDS        4 waves x 2 x 16 KiB = 128 KiB in the loop; the merge needs 32 x (256 + 4) x 4 = 33 280 bytes per wave, so a wave's region is
//              34 KiB and the kernel takes 136 KiB + 1 KiB of (m, l): one workgroup per CU, as at d = 128
//   loads      16 (K) + 16 (V) = 32 per lane and block: "only the next block's loads are outstanding" is vmcnt(32), inside the 6 bits
//   registers  Q 64 + K 128 + O 128 + row sum 16 + scores 16 + P 16, plus the V^T fragments in flight: one wave per SIMD at 512, no scratch
// Paged: a 32-key block lies in at most two 16-row pages, so a wave holds TWO table entries per block (wave-uniform, scalar loads through the
// constant address space), fetched two blocks ahead of the loads that use them.
#pragma once
#include "fa_kv_decode_core.h"
#include "fa_kv256.h"

namespace fa {

struct Kv256Cfg {
    static constexpr int D = kKv256HeadDim, KS = D / 16, DB = D / 32;
    static constexpr int kBlk = 32;                          // keys per block: one MFMA row block
    static constexpr int kBlockPages = kBlk / kPagedMinPage;  // table entries of one block
    static constexpr int kVImage = kBlk * 2 * D;             // bytes of one V image
    static constexpr int kVChunk = 4;                        // column blocks of O whose V^T fragments are read together
    static constexpr int kLoadsPerBlock = KS + kVImage / 1024;   // vector-memory instructions per lane and block
    static constexpr int kMergeBytes = kKvRowTile * kKvMergeStride(D) * 4;
    static constexpr int kWaveLds = ((2 * kVImage > kMergeBytes ? 2 * kVImage : kMergeBytes) + 1023) / 1024 * 1024;   // the larger of loop and merge
    static_assert(kLoadsPerBlock <= 63, "vmcnt holds 6 bits");
    static_assert(kKvWaves * kWaveLds + 2 * kKvWaves * kKvRowTile * 4 <= 160 * 1024, "the LDS of a CU");
    static_assert(kKvBlk % kBlk == 0 && kBlk % kPagedMinPage == 0, "blocks start where shares do, and pages do not straddle them");
};

// kv_mask_and_max (fa_kv_decode_core.h) over ONE 32-key row block.  rel = lim - kv0 - 4 * hi: key offset (r & 3) + 8 * (r >> 2) > rel is not
// visible; WINDOW: rel_lo = (diag + i - window_left) - kv0 - 4 * hi, neither is an offset < rel_lo.
template <bool WINDOW>
__device__ __forceinline__ KvRescale kv256_mask_and_max(f32x16& s, int rel, float c, float& m, int rel_lo)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float t = ((r & 3) + 8 * (r >> 2) > rel) ? -INFINITY : s[r] * c;
        if constexpr (WINDOW) t = ((r & 3) + 8 * (r >> 2) < rel_lo) ? -INFINITY : t;
        s[r] = t;
    }
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[r]);
    mx = xhalf_max(mx);
    const float m_new = fmaxf(m, mx);
    const float m_use = (m_new == -INFINITY) ? 0.0f : m_new;   // a row that has seen no key yet: p = 0, no NaN
    const float alpha = fast_exp2(m - m_use);
    m = m_new;
    return KvRescale{m_use, alpha};
}

// kv_p_terms over one row block: the two B operands (16 keys each) of P.V, hi and lo
__device__ __forceinline__ void kv256_p_terms(const f32x16& s, float m_use, bf16x8 (&ph)[2], bf16x8 (&pl)[2])
{
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float pe = fast_exp2(s[8 * t + e] - m_use);
            const __bf16 h = (__bf16)pe;
            ph[t][e] = h;
            pl[t][e] = (__bf16)(pe - (float)h);
        }
}

// The page walk of fa_kv_decode_core.h for a block of two 16-row groups: the entries of the block that starts at key kv0 (only called with
// kend >= 1; the row is clamped to [lo, kend - 1] BEFORE the lookup, so no entry outside [lo >> shift, ceil(len / page)) is read) ...
template <bool WINDOW>
__device__ __forceinline__ void kv256_fetch_pages(cst_i32_t* tbl, int page_shift, int kv0, int kend, int (&e)[Kv256Cfg::kBlockPages], int lo)
{
#pragma unroll
    for (int i = 0; i < Kv256Cfg::kBlockPages; ++i) {
        int row = min(kv0 + i * kPagedMinPage, kend - 1);
        if constexpr (WINDOW) row = max(row, lo);
        int idx = __builtin_amdgcn_readfirstlane(row) >> page_shift;
        asm volatile("" : "+s"(idx));   // behind the step's last drain of the scalar counter
        e[i] = tbl[idx];
    }
}
// ... and the point up to which they must have arrived: the page offsets, in elements
__device__ __forceinline__ void kv256_pages_landed(int (&e)[Kv256Cfg::kBlockPages], int64_t page_stride, int64_t (&pb)[Kv256Cfg::kBlockPages])
{
#pragma unroll
    for (int i = 0; i < Kv256Cfg::kBlockPages; ++i) asm volatile("" : "+s"(e[i]));
#pragma unroll
    for (int i = 0; i < Kv256Cfg::kBlockPages; ++i) pb[i] = (int64_t)e[i] * page_stride;
}

template <bool CAUSAL, bool OUT_F32, bool PAGED, bool WINDOW>
__device__ __forceinline__ void kv256_decode(const Kv256Params& wp)
{
    using C = Kv256Cfg;
    constexpr int D = C::D, KS = C::KS, DB = C::DB, BLK = C::kBlk, NP = C::kBlockPages;
    __shared__ __attribute__((aligned(1024))) char smem[kKvWaves * C::kWaveLds];
    __shared__ float m_s[kKvWaves][kKvRowTile], l_s[kKvWaves][kKvRowTile];

    const PagedParams& pp = wp.pp;
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
    // Only the matrix pipe reads Q, and it takes an operand from either half of the register file: the accumulation half holds O, the row sum,
    // the scores and Q (224 of 256), the other half K's two sets, P and the V^T fragments.  Left to itself hipcc keeps Q where K is and spills.
    auto q_in_acc_half = [&]() {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+a"(qf[ks]));
    };
    q_in_acc_half();
    bf16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;

    const __bf16 *kg, *vg;
    cst_i32_t* tbl = nullptr;
    int page_mask = 0;
    unsigned row_stride = 0;
    if constexpr (PAGED) {
        kg = (const __bf16*)p.k + (int64_t)tl.head * pp.head_stride;
        vg = (const __bf16*)p.v + (int64_t)tl.head * pp.head_stride;
        tbl = (cst_i32_t*)(pp.table + (int64_t)tl.seq * pp.max_pages);
        page_mask = (1 << pp.page_shift) - 1;
        row_stride = (unsigned)pp.row_stride;
    } else {
        kg = (const __bf16*)p.k + (int64_t)tl.slab * p.kv_slab_stride;
        vg = (const __bf16*)p.v + (int64_t)tl.slab * p.kv_slab_stride;
    }
    char* vbuf = smem + wave * C::kWaveLds;
    const int li = lane & 15;
    // this lane's corner of a V^T fragment in the V image ([key/4][col/16][4][16] sub-tiles, keys permuted like the scores)
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

    // the row of the cache that key `key` of the block at kv0 loads: itself inside [lo, kend), the nearest row of that range outside
    auto row_of = [&](int key) {
        int row = min(key, kend - 1);
        if constexpr (WINDOW) row = max(row, lo);
        return row;
    };
    // Addresses are a uniform 64-bit base plus a 32-bit byte offset per lane (a slab stays below 2^32 bytes, and so does the offset inside a
    // page: the host checks both), so a load costs one address register, not two per piece.
    // The K fragments of the block that starts at key kv0: lane (lq, hi) holds columns 16 ks + 8 hi .. + 8 of key kv0 + lq.  pb: its page offsets
    auto load_k = [&](int kv0, const int64_t(&pb)[NP], bf16x8(&kf)[KS]) {
        const int row = row_of(kv0 + lq);
        const char* kr;
        if constexpr (PAGED)   // (a select between the two array elements themselves becomes an indexed read of the array: scratch)
            kr = (const char*)(kg + pb[0] + ((lq & 16) ? pb[1] - pb[0] : (int64_t)0)) + ((unsigned)(row & page_mask) * row_stride + hi * 8) * 2u;
        else
            kr = (const char*)kg + ((unsigned)row * (unsigned)(2 * D) + hi * 16);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[ks] = *(const bf16x8*)(kr + ks * 32);
    };
    // ... and its V image: sixteen 1 KiB pieces, each half a 4-key group (8 sub-tiles of 4 keys x 16 columns); piece ch holds keys
    // 4 (ch / 2) .. + 4, so its 16-row page group ch / 8 is the same in every lane
    const int v_key = (lane % 8) / 2, v_col = (lane / 8) * 16 + (lane & 1) * 8;   // this lane's key and column within pieces 0 and 1
    auto issue_v = [&](int kv0, const int64_t(&pb)[NP], char* dst) {
#pragma unroll
        for (int ch = 0; ch < C::kVImage / 1024; ++ch) {
            const int row = row_of(kv0 + (ch / 2) * 4 + v_key);
            const int col = (ch & 1) * (D / 2) + v_col;
            const char* src;
            if constexpr (PAGED)
                src = (const char*)(vg + pb[ch / 8]) + ((unsigned)(row & page_mask) * row_stride + col) * 2u;
            else
                src = (const char*)vg + ((unsigned)row * (unsigned)(2 * D) + col * 2);
            __builtin_amdgcn_global_load_lds((gbl_cvoid_t*)src, (lds_void_t*)(dst + ch * 1024), 16, 0, 0);
        }
    };

    // One block.  The K fragments ping-pong between two register sets by NAME (the loop below is unrolled by two): a copy "current = next" at
    // the end of a step would have to wait for the next block's loads.
    // PAGED: the table runs two blocks ahead of the loads: pg[] holds the page offsets of the block whose loads the next step issues, ent[] the
    // entries of the block after that, in flight from the end of one step to the end of the next.
    int64_t pg[NP];
    int ent[NP];
    auto step = [&](int blk, int par, const bf16x8(&kcur)[KS], bf16x8(&knext)[KS]) __attribute__((always_inline)) {
        const int kv0 = kbeg + blk * BLK;
        // The wave's next block, unconditionally: K to the spare registers, V to the other image.  Past the share's end every lane's row is
        // redirected to the share's last row (one cached row per load), so the last step costs no traffic, the loop body has no branch, and
        // the number of loads in flight is the same in every step -- which is what lets the wait below count.
        load_k(kv0 + kKvWaves * BLK, pg, knext);
        issue_v(kv0 + kKvWaves * BLK, pg, vbuf + (par ^ 1) * C::kVImage);

        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kcur[ks], qf[ks], s, 0, 0, 0);

        bf16x8 ph[2], pl[2];
        const KvRescale rs = kv256_mask_and_max<WINDOW>(s, lim - kv0 - 4 * hi, c, m, lo_row - kv0 - 4 * hi);
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] *= rs.alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) lacc[r] *= rs.alpha;
        kv256_p_terms(s, rs.m_use, ph, pl);

        // this block's V image has landed once only the next block's loads are outstanding
        wait_vm_outstanding<C::kLoadsPerBlock>();
        const unsigned v_addr = (unsigned)(size_t)(lds_void_t*)(vbuf + par * C::kVImage + v_lane_off);
#pragma unroll
        for (int t = 0; t < 2; ++t) {   // 16 keys: key groups 4 t + hi and 4 t + 2 + hi
#pragma unroll
            for (int d0 = 0; d0 < DB; d0 += C::kVChunk) {   // kVChunk column blocks of O at a time: the fragments in flight stay few
                s16x4 vv[2 * C::kVChunk];
#pragma unroll
                for (int i = 0; i < C::kVChunk; ++i) {
                    vv[2 * i] = lds_read_tr16(v_addr + ((4 * t + 0) * (D / 16) + 2 * (d0 + i)) * 128);
                    vv[2 * i + 1] = lds_read_tr16(v_addr + ((4 * t + 2) * (D / 16) + 2 * (d0 + i)) * 128);
                }
                lds_reads_landed(vv);
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
            kv256_pages_landed(ent, pp.page_stride, pg);                                                // the block the next step issues: fetched a step ago
            kv256_fetch_pages<WINDOW>(tbl, pp.page_shift, kv0 + 3 * kKvWaves * BLK, kend, ent, lo);     // the block after that
        }
        q_in_acc_half();
        asm volatile("" ::: "memory");   // the image is read before the next step's DMA may be enqueued over its twin
    };

    bf16x8 kc[KS], kn[KS];
#pragma unroll
    for (int i = 0; i < NP; ++i) pg[i] = 0, ent[i] = 0;
    if (wave < nblk) {   // kend >= 1 from here on: every row (and, PAGED, every table index) is that of a key below len
        if constexpr (PAGED) {
            int e0[NP], e1[NP];
            kv256_fetch_pages<WINDOW>(tbl, pp.page_shift, kbeg + wave * BLK, kend, e0, lo);
            kv256_fetch_pages<WINDOW>(tbl, pp.page_shift, kbeg + (wave + kKvWaves) * BLK, kend, e1, lo);
            int64_t p0[NP];
            kv256_pages_landed(e0, pp.page_stride, p0);
            load_k(kbeg + wave * BLK, p0, kc);
            issue_v(kbeg + wave * BLK, p0, vbuf);
            kv256_pages_landed(e1, pp.page_stride, pg);
            kv256_fetch_pages<WINDOW>(tbl, pp.page_shift, kbeg + (wave + 2 * kKvWaves) * BLK, kend, ent, lo);
        } else {
            load_k(kbeg + wave * BLK, pg, kc);
            issue_v(kbeg + wave * BLK, pg, vbuf);
        }
    }
    asm volatile("" ::: "memory");
    for (int blk = wave; blk < nblk; blk += 2 * kKvWaves) {
        step(blk, 0, kc, kn);
        if (blk + kKvWaves < nblk) step(blk + kKvWaves, 1, kn, kc);
    }

    mfma_drain();     // the loop exit is a branch: the last matrix instructions may still be in flight
    wait_lds_dma();   // the last step's look-ahead still targets an image; after it the merge may take the wave's region
    // hipcc cannot see that wait (it is inline asm): one it can see keeps its own, for the look-ahead K registers the merge overwrites, at the
    // top of the merge whatever the register allocation is
    __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0) alone
    __builtin_amdgcn_sched_barrier(0);
    kv_merge_and_store<D, OUT_F32, false, C::kWaveLds>(p, tl, smem, m_s, l_s, wave, lq, hi, m, o, lacc, 1.0f);
}

}  // namespace fa
