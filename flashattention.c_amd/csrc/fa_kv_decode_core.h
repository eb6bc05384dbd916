// fa_kv_decode_core.h -- the device pieces the decode kernels of the KV-cache libraries are made of: few query rows against many cached
// keys (decode, chunked prefill, cross-attention, GQA), the bandwidth-bound twin of the square kernels.  No counterpart in the reference, whose
// one entry computes square self-attention.  Users: fa_kv_decode16_body.h (the 16-bit loop of fa_kv_decode.hip, fa_paged_decode.hip and, with
// WINDOW = true, fa_kvw_decode.hip) and fa_kv8_decode_body.h (the fp8 loop of fa_kv8_decode.hip and, with WINDOW = true, fa_kvw8_decode.hip).  Every piece is forced inline; nothing here branches at run time on the kind of
// cache, and what a sliding window adds sits behind `if constexpr (WINDOW)`: with WINDOW = false (the default of every piece) the text is
// what it was.
//
// The pieces return values and take values (not references to the kernel's arguments or accumulators) wherever they can, and the kernels keep
// what hipcc compiles to other code once it is a function of its own -- the empty share's `return`, the rescale of the accumulators, the P.V
// sequence: tests/test_kv_code_profile.py holds every kernel to the instruction profile it had when these pieces were written out in it.
//
// A workgroup owns (K/V slab, row tile, key share).  The M = group * nq query rows that share one K/V slab are contiguous in q / o
// ("packed rows": row r is query i = r % nq of head g = r / nq), a row tile is 32 of them -- one column block of the swapped product
// S^T = K Q^T (v_mfma_f32_32x32x16_bf16), so a lane holds 32 scores of ONE row and the row maximum is in-lane plus one
// v_permlane32_swap -- and K/V are read once per row tile, not once per query head.  The four waves walk disjoint 64-key blocks of
// the share (block = wave, wave + 4, ...), each with its own online-softmax state, and merge through LDS at the end.
// Keys at or beyond the slab's length (or the share's end, or above a row's causal diagonal) are masked to -inf before the maximum;
// their loads are redirected to the last valid row of the share, so no row >= len is ever read.
// Arithmetic: Q.K^T one bf16 product into fp32; P = bf16 hi + bf16 lo (lo = bf16 of the exact residual), V as it is; the row sum is
// accumulated by the matrix pipe too, against an all-ones A operand in the same instruction sequence as every column of O: a
// constant V comes out exactly.
//
// Paged caches (include/flashattn_amd_paged.h): K/V rows are found through a block table over a shared page pool,
//
//   row j of sequence b, head h  ->  pool + table[b][j >> page_shift] * page_stride + (j & (page - 1)) * row_stride + h * head_stride
//
// Shares and blocks start at multiples of 64 keys and pages are powers of two >= 16 rows, so a wave's 64-key block lies in at most four
// pages, and lane-independent ones: the block's entries are table[min(kv0 + 16 i, kend - 1) >> page_shift], i = 0 .. 3 (all four the same
// entry for pages of 64 rows and more, two pairs for 32).  They are wave-uniform, read through the constant address space -- scalar loads,
// counted by lgkmcnt, which the loops drain by hand anyway; vmcnt, which the 16-bit loop counts, never sees them -- and held as four uniform
// 64-bit page offsets.  A lane picks by (key >> 4): a compile-time index for every V piece, one select for a K row.  The redirect "rows past
// the share's end load the share's last row" acts on the LOGICAL row, before the lookup: entry i clamps its row to kend - 1 the same way,
// so a redirected row finds the page of row kend - 1 under the index it would have used, and no entry at or beyond ceil(len / page) is
// ever read.  The entries of a block are fetched at the end of a step, land during the next one and are used at the start of the one
// after that: no table round trip sits between two blocks' loads, and none in front of the matrix pipe.
#pragma once
#include "fa_paged.h"
#include "fa_bf16_common.h"

namespace fa {

typedef __attribute__((address_space(4))) const int32_t cst_i32_t;   // a load through it is a scalar load wherever its address is uniform
static_assert(kPagedBlockPages * kPagedMinPage == kKvBlk, "the entries of one block");

// ---- the workgroup's tile ----
struct KvTile {
    int s_idx, tile, slab;   // key share, row tile, K/V slab: share fastest, so the shares of a row tile run side by side
    int seq, head;           // the slab's sequence and its head in it (a contiguous cache: the slab itself, 0)
    int len;                 // keys of the slab's sequence
    int diag;                // len - nq.  Causal is bottom-right aligned: query i sees keys j <= diag + i
    int row0;                // first packed row of the tile within its slab
    int kbeg, kend, nblk;    // the keys [kbeg, kend) this workgroup reads, in nblk 64-key blocks
    int lo;                  // WINDOW: the tile's lowest visible key (kbeg <= lo only in the tile's first share); 0 otherwise
    int64_t rows_total;      // packed rows over all slabs
    int64_t prow0;           // first packed row of the tile, over all slabs
};

// heads_kv: the slabs that share one length (and, paged, one table): 1 for a contiguous cache, the K/V heads of a sequence for a paged one.
// WINDOW (the sliding-window kernels of fa_kvw_decode.hip; include/flashattn_amd_kvw.h): query i sees no key below diag + i - window_left.
// The tile's lowest visible key is lo = max(0, diag + imin - window_left), imin the smallest query index among the tile's rows, and the
// shares are laid over the keys from lo & ~63 on instead of from 0 -- blocks still start at multiples of 64 keys.
template <bool CAUSAL, bool WINDOW = false>
__device__ __forceinline__ KvTile kv_tile(const KvParams& p, int heads_kv, int window_left = 0)
{
    const int s_idx = blockIdx.x % p.splits;
    const int tile = (blockIdx.x / p.splits) % p.row_tiles;
    const int slab = blockIdx.x / (p.splits * p.row_tiles);
    const int M = p.m_rows, nq = p.nq;

    const int seq = slab / heads_kv, head = slab % heads_kv;

    int len = p.nk;
    if (p.kv_lens != nullptr) len = min(max(p.kv_lens[seq], 0), p.nk);

    const int row0 = tile * kKvRowTile, rlast = min(row0 + kKvRowTile - 1, M - 1);
    const int diag = len - nq;
    int kbeg = s_idx * p.share, lo = 0;
    if constexpr (WINDOW) {
        const int imin = (row0 / nq != rlast / nq) ? 0 : row0 % nq;
        lo = max(diag + imin - window_left, 0);
        kbeg += lo & ~(kKvBlk - 1);
    }
    int kend = min(kbeg + p.share, len);
    if (CAUSAL) {   // the tile's widest row bounds what the workgroup reads
        const int imax = (row0 / nq != rlast / nq) ? nq - 1 : rlast % nq;
        kend = min(kend, diag + imax + 1);
    }
    const int64_t rows_total = (int64_t)p.bh_kv * M;
    const int64_t prow0 = (int64_t)slab * M + row0;
    const int nblk = kend > kbeg ? (kend - kbeg + kKvBlk - 1) / kKvBlk : 0;
    return KvTile{s_idx, tile, slab, seq, head, len, diag, row0, kbeg, kend, nblk, lo, rows_total, prow0};
}

// The share lies beyond len or above the tile's diagonal: the kernel says so in the share's LSE partial and returns -- its O partial stays
// unwritten, the combine drops it.  (Test and store are two functions so that the exit is a plain branch of the kernel.)
__device__ __forceinline__ bool kv_share_is_empty(const KvParams& p, const KvTile& t) { return t.nblk == 0 && p.splits > 1; }
__device__ __forceinline__ void kv_mark_share_empty(const KvParams& p, const KvTile& t)
{
    if (threadIdx.x < kKvRowTile && t.row0 + (int)threadIdx.x < p.m_rows) p.lse_part[(int64_t)t.s_idx * t.rows_total + t.prow0 + threadIdx.x] = -INFINITY;
}

// lane lq's row of the tile: is it a row of the slab, and the last key it sees
__device__ __forceinline__ bool kv_row_ok(const KvParams& p, const KvTile& t, int lq) { return t.row0 + lq < p.m_rows; }
template <bool CAUSAL>
__device__ __forceinline__ int kv_last_visible_key(const KvParams& p, const KvTile& t, int lq)
{
    int lim = t.kend - 1;
    if (CAUSAL) lim = min(lim, t.diag + (t.row0 + lq) % p.nq);
    return lim;
}

// ---- Q fragment ks of lane (lq, hi): the B operand of K Q^T, 8 consecutive columns of the lane's row per 16-column step ----
template <int D>
__device__ __forceinline__ bf16x8 kv_q_fragment(const void* q, int64_t prow0, bool row_ok, int lq, int hi, int ks)
{
    const bf16x8 f = *(const bf16x8*)((const __bf16*)q + (prow0 + (row_ok ? lq : 0)) * D + hi * 8 + ks * 16);
    const bf16x8 zeros = {};
    return row_ok ? f : zeros;   // rows past M: computed on zeros, never stored
}

// ---- one block's softmax step, in two pieces with the rescale of the accumulators between them in the kernel ----
// first: exp2 domain, mask (branch-free: the vector ALU idles in these kernels), row maximum; s becomes the masked scores, m the new maximum.
// rel = lim - kv0 - 4 * hi: key offset (kb * 32 + (r & 3) + 8 * (r >> 2)) > rel is not visible
// WINDOW: rel_lo = (diag + i - window_left) - kv0 - 4 * hi: neither is a key offset < rel_lo -- one more select on the score, no branch
struct KvRescale {
    float m_use;   // what the exponentials of this block refer to
    float alpha;   // what the accumulators are multiplied by
};
template <bool WINDOW = false>
__device__ __forceinline__ KvRescale kv_mask_and_max(f32x16 (&s)[2], int rel, float c, float& m, int rel_lo = 0)
{
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float t = (kb * 32 + (r & 3) + 8 * (r >> 2) > rel) ? -INFINITY : s[kb][r] * c;
            if constexpr (WINDOW) t = (kb * 32 + (r & 3) + 8 * (r >> 2) < rel_lo) ? -INFINITY : t;
            s[kb][r] = t;
        }
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kb][r]);
    mx = xhalf_max(mx);
    const float m_new = fmaxf(m, mx);
    const float m_use = (m_new == -INFINITY) ? 0.0f : m_new;   // a row that has seen no key yet: p = 0, no NaN
    const float alpha = fast_exp2(m - m_use);
    m = m_new;
    return KvRescale{m_use, alpha};
}
// second: P = bf16 hi + bf16 lo of 2^(s - m_use), as the four B operands of P.V
__device__ __forceinline__ void kv_p_terms(const f32x16 (&s)[2], float m_use, bf16x8 (&ph)[4], bf16x8 (&pl)[4])
{
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float pe = fast_exp2(s[kb][8 * t + e] - m_use);
                const __bf16 h = (__bf16)pe;
                ph[kb * 2 + t][e] = h;
                pl[kb * 2 + t][e] = (__bf16)(pe - (float)h);
            }
}

constexpr int kKvMergeStride(int d) { return d + 4; }   // floats per row of a wave's O in the merge (padded against bank conflicts)

// ---- merge of the four waves, (m, l, O) of each through LDS, and the epilogue ----
// smem: kKvWaves regions of WAVE_LDS bytes, each at least 32 rows of kKvMergeStride(D) floats and no longer in use (the caller has drained
// the matrix pipe and whatever still targets the region).  SCALED: the normalised row is multiplied by v_scale before the store to o -- behind
// the quotient, so a constant V comes out as exactly v_scale x it -- on the unsplit path only: partial outputs stay unscaled, the merge
// kernel multiplies behind ITS quotient (fa_kv_combine_kernel.h says why).  The LSE is that of the scaled scores: no v_scale.
template <int D, bool OUT_F32, bool SCALED, int WAVE_LDS>
__device__ __forceinline__ void kv_merge_and_store(const KvParams& p, const KvTile& t, char* smem, float (&m_s)[kKvWaves][kKvRowTile],
                                                   float (&l_s)[kKvWaves][kKvRowTile], int wave, int lq, int hi, float m, const f32x16 (&o)[D / 32],
                                                   const f32x16& lacc, float v_scale)
{
    constexpr int DB = D / 32, kStride = kKvMergeStride(D);
    static_assert(kKvRowTile * kStride * 4 <= WAVE_LDS, "a wave's partial O must fit its own region");
    {
        float* ow = (float*)(smem + wave * WAVE_LDS) + lq * kStride + 4 * hi;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 pk;
#pragma unroll
                for (int e = 0; e < 4; ++e) pk[e] = o[db][4 * g + e];
                *(f32x4*)(ow + db * 32 + 8 * g) = pk;
            }
        if (hi == 0) {
            m_s[wave][lq] = m;
            l_s[wave][lq] = lacc[0];
        }
    }
    __syncthreads();

    const int row = threadIdx.x >> 3, j = threadIdx.x & 7;   // 8 threads per row, D / 32 four-column pieces each
    if (t.row0 + row >= p.m_rows) return;
    float mw[kKvWaves], a[kKvWaves];
    float mt = -INFINITY;
#pragma unroll
    for (int w = 0; w < kKvWaves; ++w) {
        mw[w] = m_s[w][row];
        mt = fmaxf(mt, mw[w]);
    }
    float lt = 0.0f;
#pragma unroll
    for (int w = 0; w < kKvWaves; ++w) {
        a[w] = (mw[w] == -INFINITY) ? 0.0f : fast_exp2(mw[w] - mt);
        lt = __builtin_fmaf(a[w], l_s[w][row], lt);
    }
    const bool none = !(lt > 0.0f);   // no visible key in this share: O = 0, LSE = -inf
    const int64_t prow = t.prow0 + row;
    const int64_t orow = (p.splits > 1 ? (int64_t)t.s_idx * t.rows_total : 0) + prow;
#pragma unroll
    for (int i = 0; i < DB; ++i) {
        const int col = (j + 8 * i) * 4;
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int w = 0; w < kKvWaves; ++w) {
            const f32x4 x = *(const f32x4*)((const float*)(smem + w * WAVE_LDS) + row * kStride + col);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(a[w], x[e], acc[e]);   // the same operation sequence as lt: acc == lt where V is constant 1
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = none ? 0.0f : acc[e] / lt;
        if (p.splits > 1) {
            *(f32x4*)(p.o_part + orow * D + col) = acc;
            continue;
        }
        if constexpr (SCALED)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] *= v_scale;
        if (OUT_F32) {
            *(f32x4*)((float*)p.o + orow * D + col) = acc;
        } else {
            bf16x4 r;
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = (__bf16)acc[e];
            *(bf16x4*)((__bf16*)p.o + orow * D + col) = r;
        }
    }
    if (j == 0) {
        const float lse = none ? -INFINITY : (mt + __builtin_amdgcn_logf(lt)) * kLn2;
        if (p.splits > 1)
            p.lse_part[orow] = lse;
        else if (p.lse != nullptr)
            p.lse[prow] = lse;
    }
}

// ---- the page walk ----
// The table entries of the block that starts at key kv0, issued back to back; only called with kend >= 1.  The empty statement pins the
// reads behind the statements before it: lgkmcnt counts them together with the LDS reads, so a read issued before the step's last
// "s_waitcnt lgkmcnt(0)" would have the matrix pipe wait for a table round trip.
// WINDOW: the row is clamped from below to the tile's lowest visible key as well, so no entry below lo >> page_shift is read either.
template <bool WINDOW = false>
__device__ __forceinline__ void fetch_pages(cst_i32_t* tbl, int page_shift, int kv0, int kend, int (&e)[kPagedBlockPages], int lo = 0)
{
#pragma unroll
    for (int i = 0; i < kPagedBlockPages; ++i) {
        int row = min(kv0 + i * kPagedMinPage, kend - 1);
        if constexpr (WINDOW) row = max(row, lo);
        int idx = __builtin_amdgcn_readfirstlane(row) >> page_shift;
        asm volatile("" : "+s"(idx));
        e[i] = tbl[idx];
    }
}
// ... and the point up to which they must have arrived: the end of the NEXT step, behind that step's drains of the scalar counter.  The
// empty statements keep the compiler from using an entry (and so from waiting for it) any earlier.  Then the page offsets, in elements.
__device__ __forceinline__ void pages_landed(int (&e)[kPagedBlockPages], int64_t page_stride, int64_t (&pb)[kPagedBlockPages])
{
#pragma unroll
    for (int i = 0; i < kPagedBlockPages; ++i) asm volatile("" : "+s"(e[i]));
#pragma unroll
    for (int i = 0; i < kPagedBlockPages; ++i) pb[i] = (int64_t)e[i] * page_stride;
}
// the page offset of key kb * 32 + lq of a block: 16-key group 2 kb + (lq >> 4)
// (a select between the two array elements themselves becomes an indexed read of the array: scratch)
__device__ __forceinline__ int64_t page_of_k_row(const int64_t (&pb)[kPagedBlockPages], int kb, int lq)
{
    return pb[2 * kb] + ((lq & 16) ? pb[2 * kb + 1] - pb[2 * kb] : (int64_t)0);
}

// ---- helpers of the 16-bit loop ----
template <int D>
struct KvCfg {
    static constexpr int KS = D / 16, DB = D / 32;
    static constexpr int kVTile = kKvBlk * 2 * D;          // bytes of one V image (64 keys)
    static constexpr int kWaveLds = 2 * kVTile;            // two images per wave
    static constexpr int kLoadsPerBlock = 2 * KS + kVTile / 1024;   // vector-memory instructions per lane and block: K fragments + V pieces
    static_assert(kLoadsPerBlock <= 63, "vmcnt holds 6 bits");   // what the loop waits for: "only the next block's loads are outstanding"
};

// issue_v_tile<D, 1> (fa_bf16_common.h, which the product kernels compile and which stays as it is) with the window's lower clamp: rows
// below lo load row lo, rows at or beyond n load row n - 1.  The same pieces, the same order, the same addresses for rows inside [lo, n).
template <int D>
__device__ __forceinline__ void issue_v_tile_from(const __bf16* __restrict__ vg, int kv0, int lo, int n, char* dst, int lane)
{
#pragma unroll
    for (int ch = 0; ch < kKvBlk * 2 * D / 1024; ++ch) {
        const int blk = ch * 8 + lane / 8;
        const int kg4 = blk / (D / 16), cb = blk % (D / 16);
        const int key = kg4 * 4 + (lane % 8) / 2;
        const int col = cb * 16 + (lane & 1) * 8;
        const int grow = max(min(kv0 + key, n - 1), lo);
        const __bf16* src = vg + (int64_t)grow * D + col;
        __builtin_amdgcn_global_load_lds((gbl_cvoid_t*)src, (lds_void_t*)(dst + ch * 1024), 16, 0, 0);
    }
}

template <int N>
__device__ __forceinline__ void wait_vm_outstanding() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// The V^T fragments are read from inline asm.  hipcc cannot tell which of a wave's two V images an LDS read touches, and puts "wait for
// EVERY LDS-DMA in flight" in front of each LDS read it can see -- which would wait for the next block's loads as well and leave nothing in
// flight while a block is computed.  The 16-bit loop waits by count (wait_vm_outstanding) for exactly the image it is about to read.
__device__ __forceinline__ s16x4 lds_read_tr16(unsigned addr)
{
    s16x4 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(addr) : "memory");
    return v;
}
// ... so their completion is waited for by hand too: nothing the compiler schedules may use vv[] before this point
template <int N>
__device__ __forceinline__ void lds_reads_landed(s16x4 (&vv)[N])
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < N; ++i) asm volatile("" : "+v"(vv[i]));
}

}  // namespace fa
