// fa_paged_decode.hip -- the paged twin of fa_kv_decode.hip: the same workgroup, loop and arithmetic, with K/V rows found through a block
// table over a shared page pool (include/flashattn_amd_paged.h).  No counterpart in the reference.  The loop body is a copy of
// fa_kv_decode.hip's (that file is left untouched: its device code is pinned); what differs is how a row's address is formed:
//
//   row j of sequence b, head h  ->  pool + table[b][j >> page_shift] * page_stride + (j & (page - 1)) * row_stride + h * head_stride
//
// Table reads.  Shares and blocks start at multiples of 64 keys and pages are powers of two >= 16 rows, so a wave's 64-key block lies in
// at most four pages, and lane-independent ones: the block's entries are table[min(kv0 + 16 i, kend - 1) >> page_shift], i = 0 .. 3 (all
// four the same entry for pages of 64 rows and more, two pairs for 32).  They are wave-uniform, read through the constant address space --
// scalar loads, counted by lgkmcnt, which the loop drains by hand anyway; vmcnt, which the loop counts, never sees them -- and held
// as four uniform 64-bit page offsets.  A lane picks by (key >> 4): a compile-time index for every V piece, one select for a K row.
// The redirect "rows past the share's end load the share's last row" acts on the LOGICAL row, before the lookup: entry i clamps its row
// to kend - 1 the same way, so a redirected row finds the page of row kend - 1 under the index it would have used, and no entry at or
// beyond ceil(len / page) is ever read.  The entries of a block are fetched at the end of a step, land during the next one and are used at
// the start of the one after that: no table round trip sits between two blocks' loads, and none in front of the matrix pipe.
//
// As in fa_kv_decode.hip: a workgroup owns (K/V slab, row tile, key share).  The M = group * nq query rows that share one K/V slab are contiguous in q / o
// ("packed rows": row r is query i = r % nq of head g = r / nq), a row tile is 32 of them -- one column block of the swapped product
// S^T = K Q^T (v_mfma_f32_32x32x16_bf16), so a lane holds 32 scores of ONE row and the row maximum is in-lane plus one
// v_permlane32_swap -- and K/V are read once per row tile, not once per query head.  The four waves walk disjoint 64-key blocks of
// the share (block = wave, wave + 4, ...), each with its own online-softmax state, and merge through LDS at the end.
//
// Data movement, per wave and 64-key block:
//   K  straight to registers: the A operand of K Q^T is "lane (key, half) holds 8 consecutive columns of its key", i.e. one 16-byte
//      load per lane and 16 columns -- an operand streamed once gains nothing from an LDS round trip
//   V  the second product contracts over keys and needs V^T fragments; those come from ds_read_b64_tr_b16 over the V image of
//      fa_bf16_common.h, which LDS-DMA (16 bytes per lane, no register staging) fills.  Two images per wave: block j + 1 (K registers
//      and V image) is in flight while block j is computed -- 4 waves x 32 KiB at d = 128, and the buffers are private to a wave, so
//      the loop has no barrier.
// Keys at or beyond the slab's length (or the share's end, or above a row's causal diagonal) are masked to -inf before the maximum;
// their loads are redirected to the last valid row of the share, so no row >= len is ever read.
// Arithmetic: Q.K^T one bf16 product into fp32; P = bf16 hi + bf16 lo (lo = bf16 of the exact residual), V as it is; the row sum is
// accumulated by the matrix pipe too, against an all-ones A operand in the same instruction sequence as every column of O: a
// constant V comes out exactly.
#include "fa_paged.h"
#include "fa_bf16_common.h"

namespace fa {

typedef __attribute__((address_space(4))) const int32_t cst_i32_t;   // a load through it is a scalar load wherever its address is uniform
static_assert(kPagedBlockPages * kPagedMinPage == kKvBlk, "the entries of one block");

template <int D>
struct KvCfg {
    static constexpr int KS = D / 16, DB = D / 32;
    static constexpr int kVTile = kKvBlk * 2 * D;          // bytes of one V image (64 keys)
    static constexpr int kWaveLds = 2 * kVTile;            // two images per wave
    static constexpr int kLoadsPerBlock = 2 * KS + kVTile / 1024;   // vector-memory instructions per lane and block: K fragments + V pieces
    static constexpr int kMergeStride = D + 4;             // floats per row of a wave's O in the merge (padded against bank conflicts)
    static_assert(32 * kMergeStride * 4 <= kWaveLds, "a wave's partial O must fit its own V images");
    static_assert(kLoadsPerBlock <= 63, "vmcnt holds 6 bits");   // what the loop waits for: "only the next block's loads are outstanding"
};

template <int N>
__device__ __forceinline__ void wait_vm_outstanding() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// The V^T fragments are read from inline asm.  hipcc cannot tell which of a wave's two V images an LDS read touches, and puts "wait for
// EVERY LDS-DMA in flight" in front of each LDS read it can see -- which would wait for the next block's loads as well and leave nothing in
// flight while a block is computed.  The loop below waits by count (wait_vm_outstanding) for exactly the image it is about to read.
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

template <int D, bool CAUSAL, bool OUT_F32>
__global__ __launch_bounds__(kKvWaves* kWave) void fa_paged_decode_kernel(PagedParams pp)
{
    const KvParams& p = pp.kv;
    constexpr int NP = kPagedBlockPages;
    using C = KvCfg<D>;
    constexpr int KS = C::KS, DB = C::DB;
    __shared__ __attribute__((aligned(1024))) char smem[kKvWaves * C::kWaveLds];
    __shared__ float m_s[kKvWaves][kKvRowTile], l_s[kKvWaves][kKvRowTile];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lq = lane & 31, hi = lane >> 5;

    // share fastest: the shares of a row tile run side by side
    const int s_idx = blockIdx.x % p.splits;
    const int tile = (blockIdx.x / p.splits) % p.row_tiles;
    const int slab = blockIdx.x / (p.splits * p.row_tiles);
    const int M = p.m_rows, nq = p.nq;

    const int seq = slab / pp.heads_kv, head = slab % pp.heads_kv;   // one table and one length per sequence, shared by its heads

    int len = p.nk;
    if (p.kv_lens != nullptr) len = min(max(p.kv_lens[seq], 0), p.nk);

    const int row0 = tile * kKvRowTile, rlast = min(row0 + kKvRowTile - 1, M - 1);
    const int kbeg = s_idx * p.share;
    int kend = min(kbeg + p.share, len);
    if (CAUSAL) {   // bottom-right aligned: query i sees keys j <= len - nq + i; the tile's widest row bounds what the workgroup reads
        const int imax = (row0 / nq != rlast / nq) ? nq - 1 : rlast % nq;
        kend = min(kend, len - nq + imax + 1);
    }
    const int64_t rows_total = (int64_t)p.bh_kv * M;
    const int64_t prow0 = (int64_t)slab * M + row0;        // first packed row of the tile, over all slabs
    const int nblk = kend > kbeg ? (kend - kbeg + kKvBlk - 1) / kKvBlk : 0;

    if (nblk == 0 && p.splits > 1) {   // the share lies beyond len or above the tile's diagonal: its O partial stays unwritten, the combine drops it
        if (threadIdx.x < kKvRowTile && row0 + (int)threadIdx.x < M) p.lse_part[(int64_t)s_idx * rows_total + prow0 + threadIdx.x] = -INFINITY;
        return;
    }

    const bool row_ok = row0 + lq < M;
    int lim = kend - 1;   // last key this lane's row sees
    if (CAUSAL) lim = min(lim, len - nq + (row0 + lq) % nq);

    bf16x8 qf[KS];
    {
        const __bf16* qr = (const __bf16*)p.q + (prow0 + (row_ok ? lq : 0)) * D + hi * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            qf[ks] = *(const bf16x8*)(qr + ks * 16);
            if (!row_ok)   // rows past M: computed on zeros, never stored
#pragma unroll
                for (int e = 0; e < 8; ++e) qf[ks][e] = (__bf16)0.0f;
        }
    }
    bf16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;

    const __bf16* kg = (const __bf16*)p.k + (int64_t)head * pp.head_stride;
    const __bf16* vg = (const __bf16*)p.v + (int64_t)head * pp.head_stride;
    cst_i32_t* tbl = (cst_i32_t*)(pp.table + (int64_t)seq * pp.max_pages);
    const int page_mask = (1 << pp.page_shift) - 1;
    const unsigned row_stride = (unsigned)pp.row_stride;
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
    // The table entries of the block that starts at key kv0, issued back to back; only called with kend >= 1.  The empty statement pins the
    // reads behind the statements before it: lgkmcnt counts them together with the LDS reads, so a read issued before the step's last
    // "s_waitcnt lgkmcnt(0)" would have the matrix pipe wait for a table round trip.
    auto fetch_pages = [&](int kv0, int(&e)[NP]) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            int idx = __builtin_amdgcn_readfirstlane(min(kv0 + i * kPagedMinPage, kend - 1)) >> pp.page_shift;
            asm volatile("" : "+s"(idx));
            e[i] = tbl[idx];
        }
    };
    // ... and the point up to which they must have arrived: the end of the NEXT step, behind that step's drains of the scalar counter.  The
    // empty statements keep the compiler from using an entry (and so from waiting for it) any earlier.  Then the page offsets, in elements.
    auto pages_landed = [&](int(&e)[NP], int64_t(&pb)[NP]) {
#pragma unroll
        for (int i = 0; i < NP; ++i) asm volatile("" : "+s"(e[i]));
#pragma unroll
        for (int i = 0; i < NP; ++i) pb[i] = (int64_t)e[i] * pp.page_stride;
    };
    auto load_k = [&](int kv0, const int64_t(&pb)[NP], bf16x8(&kf)[2][KS]) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int row = min(kv0 + kb * 32 + lq, kend - 1);   // key kb * 32 + lq of the block: 16-key group 2 kb + (lq >> 4)
            // (a select between the two array elements themselves becomes an indexed read of the array: scratch)
            const int64_t page = pb[2 * kb] + ((lq & 16) ? pb[2 * kb + 1] - pb[2 * kb] : (int64_t)0);
            const __bf16* kr = kg + page + (unsigned)(row & page_mask) * row_stride + hi * 8;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) kf[kb][ks] = *(const bf16x8*)(kr + ks * 16);
        }
    };
    // issue_v_tile (fa_bf16_common.h) for one wave, through the pages: the 16-key group of a piece is the same in every lane
    auto issue_v = [&](int kv0, const int64_t(&pb)[NP], char* dst) {
#pragma unroll
        for (int ch = 0; ch < C::kVTile / 1024; ++ch) {
            const int blk = ch * 8 + lane / 8;
            const int kg4 = blk / (D / 16), cb = blk % (D / 16);
            const int key = kg4 * 4 + (lane % 8) / 2;
            const int col = cb * 16 + (lane & 1) * 8;
            constexpr int kKeysPerPiece = 512 / D;   // a 1 KiB piece holds whole rows of 2 D bytes
            static_assert(kPagedMinPage % kKeysPerPiece == 0, "a piece must not straddle a 16-key group");
            const int row = min(kv0 + key, kend - 1);
            const __bf16* src = vg + pb[ch * kKeysPerPiece / kPagedMinPage] + (unsigned)(row & page_mask) * row_stride + col;
            __builtin_amdgcn_global_load_lds((gbl_cvoid_t*)src, (lds_void_t*)(dst + ch * 1024), 16, 0, 0);
        }
    };

    // One block.  The K fragments ping-pong between two register sets by NAME (the loop below is unrolled by two): a copy "current = next" at
    // the end of a step would have to wait for the next block's loads.
    // The table runs two blocks ahead of the loads: pg[] holds the page offsets of the block whose loads the next step issues, ent[] the
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

        // exp2 domain, mask (branch-free: the vector ALU idles in this kernel), row maximum
        const int rel = lim - kv0 - 4 * hi;   // key offset (kb * 32 + (r & 3) + 8 * (r >> 2)) > rel: not visible
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float t = (kb * 32 + (r & 3) + 8 * (r >> 2) > rel) ? -INFINITY : s[kb][r] * c;
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

        bf16x8 ph[4], pl[4];
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
                    o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pl[f], o[db], 0, 0, 0);
                }
                lacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, ph[f], lacc, 0, 0, 0);
                lacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, pl[f], lacc, 0, 0, 0);
            }
        pages_landed(ent, pg);                                // the block the next step issues: fetched a step ago
        fetch_pages(kv0 + 3 * kKvWaves * kKvBlk, ent);        // the block after that
        asm volatile("" ::: "memory");   // the image is read before the next step's DMA may be enqueued over its twin
    };

#pragma unroll
    for (int i = 0; i < NP; ++i) pg[i] = 0, ent[i] = 0;
    if (wave < nblk) {   // kend >= 1 from here on: every table index is that of a row below len
        int e0[NP], e1[NP];
        fetch_pages(kbeg + wave * kKvBlk, e0);
        fetch_pages(kbeg + (wave + kKvWaves) * kKvBlk, e1);
        int64_t p0[NP];
        pages_landed(e0, p0);
        load_k(kbeg + wave * kKvBlk, p0, kc);
        issue_v(kbeg + wave * kKvBlk, p0, vbuf);
        pages_landed(e1, pg);
        fetch_pages(kbeg + (wave + 2 * kKvWaves) * kKvBlk, ent);
    }
    asm volatile("" ::: "memory");
    for (int blk = wave; blk < nblk; blk += 2 * kKvWaves) {
        step(blk, 0, kc, kn);
        if (blk + kKvWaves < nblk) step(blk + kKvWaves, 1, kn, kc);
    }

    // ---- merge of the four waves: (m, l, O) of each through LDS (the wave's own V images: nothing is in flight any more) ----
    mfma_drain();   // the loop exit is a branch: the last matrix instructions may still be in flight
    wait_lds_dma();   // the last step's look-ahead still targets an image
    {
        float* ow = (float*)vbuf + lq * C::kMergeStride + 4 * hi;
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
    if (row0 + row >= M) return;
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
    const int64_t prow = prow0 + row;
    const int64_t orow = (p.splits > 1 ? (int64_t)s_idx * rows_total : 0) + prow;
#pragma unroll
    for (int i = 0; i < DB; ++i) {
        const int col = (j + 8 * i) * 4;
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int w = 0; w < kKvWaves; ++w) {
            const f32x4 x = *(const f32x4*)((const float*)(smem + w * C::kWaveLds) + row * C::kMergeStride + col);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(a[w], x[e], acc[e]);   // the same operation sequence as lt: acc == lt where V is constant 1
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = none ? 0.0f : acc[e] / lt;
        if (p.splits > 1) {
            *(f32x4*)(p.o_part + orow * D + col) = acc;
        } else if (OUT_F32) {
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

template <int D>
static hipError_t launch_decode_d(const PagedParams& pp, int causal, int out_f32, hipStream_t stream)
{
    const KvParams& p = pp.kv;
    const dim3 grid((unsigned)((int64_t)p.bh_kv * p.row_tiles * p.splits)), block(kKvWaves * kWave);
    if (causal) {
        if (out_f32)
            hipLaunchKernelGGL((fa_paged_decode_kernel<D, true, true>), grid, block, 0, stream, pp);
        else
            hipLaunchKernelGGL((fa_paged_decode_kernel<D, true, false>), grid, block, 0, stream, pp);
    } else {
        if (out_f32)
            hipLaunchKernelGGL((fa_paged_decode_kernel<D, false, true>), grid, block, 0, stream, pp);
        else
            hipLaunchKernelGGL((fa_paged_decode_kernel<D, false, false>), grid, block, 0, stream, pp);
    }
    return hipGetLastError();
}

hipError_t launch_paged_decode(const PagedParams& pp, int d, int causal, int out_f32, hipStream_t stream)
{
    if ((int64_t)pp.kv.bh_kv * pp.kv.row_tiles * pp.kv.splits > 0x7fffffffLL) return hipErrorInvalidValue;
    if (d == 64) return launch_decode_d<64>(pp, causal, out_f32, stream);
    if (d == 128) return launch_decode_d<128>(pp, causal, out_f32, stream);
    return hipErrorInvalidValue;
}

const char* paged_decode_kernel_name() { return "fa_paged_decode_kernel"; }

}  // namespace fa
