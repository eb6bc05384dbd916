// fa_kvp_prefill_loop.h -- chunked prefill over a bf16 cache at head dim 128, contiguous or paged: the kernel of libflashattn_amd_kvp.so
// (fa_kvp_prefill.hip instantiates it eight times).  The compute-bound twin of the decode loop (fa_kv_decode16_body.h): the same packed rows,
// the same masks, the same arithmetic, the opposite split of the work.  No counterpart in the reference.
// With FP8 = true it is the kernel of libflashattn_amd_kvp8.so over a cache of e4m3 bytes (fa_kvp8_prefill.hip; "FP8" below and Kvp8Map).
// With WINDOW = true it is the d = 128 kernel (either cache type) of libflashattn_amd_kvpw.so (fa_kvpw_prefill.hip, fa_kvpw8_prefill.hip; "WINDOW" below).
// Out of scope: d = 64 (d = 256: fa_kvp256_prefill_loop.h), a key split for tiny grids, routing from fa_kv_forward.
//
// Work split.  A workgroup of four waves owns (K/V slab, 256-row tile of the slab's packed rows); wave w takes rows 64 w .. 64 w + 63 of the
// tile as two 32-row blocks (nb = 0, 1).  All four waves walk the SAME 64-key blocks, from key 0 to the tile's kend = min(len, diag + imax + 1):
// no key split, no workspace, no merge.  Causal tiles are launched heaviest first.
//
// K and V through LDS, shared by the waves.  Each 64-key block is brought in once per workgroup by LDS-DMA (global_load_lds, 16 bytes per
// lane), a quarter of the 1 KiB pieces per wave: K into the row-major, slot-swizzled 16 KiB image of fa_bf16_common.h, V into its
// [key/4][col/16][4][16] image.  Two stages of (K, V): 64 KiB, one barrier per block --
//     wait for my pieces of block j;  barrier;  enqueue block j + 1 into the other stage;  compute block j
// -- the barrier says both "block j has landed in full" and "everybody is done reading block j - 1", whose stage block j + 1 overwrites.
// The DMA of block j + 1 has all of block j's arithmetic to land in, so the wait at the top (vmcnt(0): nothing else is outstanding) is free.
// The LDS reads are inline asm, counted by hand: hipcc puts "wait for EVERY LDS-DMA in flight" in front of each LDS read it can see.
// A wave reads each K fragment (ds_read_b128) and each V^T fragment (ds_read_b64_tr_b16) once and feeds it to both of its row blocks: two
// matrix instructions per LDS read, 256 rows of matrix work per K/V byte fetched (the decode kernel: 32).
//
// Registers (one wave per SIMD, 512; the code object: 256 + 236, no scratch).  O (2 x 64) and the row sums (2 x 16) live in the accumulation
// half, and hipcc puts the scores there as well.  Q is 64 registers and fits neither half beside the rest when a whole 64-key block's scores
// and P (64 + 64) are live, so a block is computed as two halves of 32 keys -- the 32-key softmax step of fa_kv256_decode_loop.h -- with 32 + 32
// live, the K fragments of a half (32) and two sets of V^T fragments (2 x 16) beside them; Q's first row block is pinned in the vector half, its
// second in the accumulation half (only the matrix pipe reads it).  The price is a second maximum / rescale test per block.
//
// Arithmetic: the contract of the KV libraries.  S^T = K Q^T on v_mfma_f32_32x32x16_bf16, one bf16 product; the mask, the maximum and the
// -inf-safe m_use of kv_mask_and_max; P = bf16 hi + bf16 lo (kv_p_terms); the row sum on the matrix pipe against all-ones in the sequence of
// every O column.  The softmax step is per 32 keys (above).  The accumulators are rescaled only in a step where some row's maximum moved (a wave-uniform branch; alpha = 1 elsewhere,
// so the bits are those of the unconditional product): they live in the accumulation half, which the vector ALU reaches through moves only.
//
// Edges: rows past M are computed on zeros and never stored; i = r % nq, so tiles and blocks may straddle heads; loads of rows at or beyond
// kend are redirected to row kend - 1 BEFORE the table lookup (fetch_pages clamps the same way); a tile without a visible key never touches
// K, V or the table and stores 0 / -inf.  A wave whose rows see nothing of a block (above its diagonal, or all past M) skips the block's matrix
// work, but still brings its pieces in and meets the barrier.
// Paged: the address rule of fa_kv_decode_core.h.  Piece i of a wave (i = 0 .. 3) holds rows 16 i + 4 wave .. + 3 of the block, so its page
// is entry i of the block's four: a compile-time index.  The entries are read through the constant address space one block ahead of the DMA
// that uses them.  A 64-bit uniform base plus a 32-bit offset per lane, under the host checks of fa_kv_host.h.
//
// FP8 (one text: everything above is compiled as it is, `if constexpr (FP8)` replaces how a block gets into a stage; with FP8 = false the
// code objects are what they were).  An e4m3 byte cannot ride the LDS-DMA: it has to pass the converter.  So
//     my stores of block j have landed (lgkmcnt(0));  barrier;  load the raw bytes of block j + 1 (four 16-byte loads per lane: 16 registers
//     held across the compute -- the code object: 256 + 253 where the bf16 kernel has 256 + 236, no scratch);  compute block j;  convert (cvt_fp8x8, exact) and store block j + 1 into the
//     other stage as eight ds_write_b128
// with block 0 loaded, converted and stored in front of the loop.  The one barrier keeps both meanings: the stage written at the end of block
// j was last read in block j - 1, which every wave left before the barrier at the top of block j.  The images are the bf16 kernel's byte for
// byte (Kvp8Map says how the lanes are laid over a block so that neither image's stores meet in a bank), so the hand-counted reads, the
// softmax halves, the matrix instructions and the epilogue are the same instructions on the same bits; v_scale multiplies once behind the
// quotient.  Against the hand-counted lgkmcnt waits of the compute: the stores are issued behind the block's last wait (lds_landed_but<0>(vb))
// and drained by the lgkmcnt(0) in front of the barrier, so none is outstanding while lds_landed_but counts reads; the paged scalar loads sit
// where the bf16 kernel has them, between the barrier and the compute, and an entry in flight only makes a counted wait stricter (above).  A
// wave's two loads of a block lie in one 16-row group each (2 i + wave / 2), so it fetches two entries per block, not four.
//
// WINDOW (one text again: everything it adds sits behind `if constexpr (WINDOW)`, and with WINDOW = false the code objects are what they
// were).  Query i sees no key below diag + i - window_left (include/flashattn_amd_kvw.h; window_left travels beside the parameter struct).
// A tile has a lower end lo beside kend -- the first key of its lowest row -- and walks the blocks lo / 64 .. nblk - 1: prologue, stage
// parity and table fetches count from there.  Rows of the first block below lo are redirected to lo as rows at or beyond kend are to kend - 1,
// on the logical row and before the table lookup, so nothing below lo is read; the mask is kv256_mask_and_max<true> with the lane's lower
// bound; and a wave skips the matrix work of a block, or of its first 32 keys, that lies wholly below its own rows' first key wbeg, as it
// does above wend.  The tile order stays: under a window the tiles weigh nearly the same.
#pragma once
#include "fa_kv256_decode_loop.h"
#include "fa_kv8_decode_core.h"
#include "fa_kvp.h"

#include <type_traits>

namespace fa {

struct KvpCfg {
    static constexpr int D = kKvpHeadDim, KS = D / 16, DB = D / 32, NB = 2;
    static constexpr int kImage = kKvBlk * 2 * D;                 // bytes of one K or V image (64 keys)
    static constexpr int kStage = 2 * kImage;                     // K, then V
    static constexpr int kPieces = kImage / 1024 / kKvWaves;      // 1 KiB DMA pieces per wave and image
    static_assert(kKvpRowTile == kKvWaves * NB * kKvRowTile, "four waves of two row blocks");
    static_assert(kPieces == kPagedBlockPages && 1024 / (2 * D) * kKvWaves == kPagedMinPage, "piece i of a wave lies in the block's 16-row group i");
    static_assert(2 * kStage <= 64 * 1024, "two stages");
};

// FP8 (fa_kvp8_prefill.hip): how a 64-key block of e4m3 bytes is split over the workgroup.  A row is 128 bytes = eight 16-byte chunks of 16
// columns; a wave-load is eight whole rows (1 KiB), and load i of wave w is rows 32 i + 8 w .. + 7 of the block for K and for V alike: inside
// ONE 16-row group, 2 i + w / 2, so the wave needs two table entries per block and both are wave-uniform.
//   K  lane l: row (l >> 3) of the eight, chunk l & 7.  The 32 bytes of bf16 are slots 2 c and 2 c + 1 of the row, kept at (2 c) ^ g and
//      (2 c) ^ g ^ 1, g = row & 15.  The eight lanes of a row write eight different slots of one 256-byte row, and the row beside them (g ^ 1)
//      the other eight: no two lanes of a ds_write_b128 pass meet in a bank.
//   V  lane l: key 4 (l >> 5) + ((l >> 1) & 3) of the eight, chunk (l & 1) + 2 ((l >> 3) & 3).  A chunk is one 32-byte row of one 128-byte
//      sub-tile, at (key / 4) * 1024 + chunk * 128 + (key % 4) * 32.  With chunk = l & 7 the eight lanes of a pass would hold ONE key and eight
//      sub-tiles 128 bytes apart: the same 32 bytes of every 256, four lanes to a bank (what v8x256_swz is for at d = 256).  Here the eight
//      consecutive lanes hold (chunk & 1, key % 4) in all eight combinations, i.e. eight different 32-byte rows of a 256-byte span, so the image
//      stays the bf16 kernel's byte for byte and its reads stay as they are: the permutation is in the loads, where it costs nothing (a
//      wave-load still covers eight whole rows).
struct Kvp8Map {
    static constexpr int kLoads = 2;                             // 16-byte loads per lane, block and tensor
    static constexpr int kRowsPerLoad = 8 * kKvWaves;            // rows of the block between a wave's two loads
    static constexpr int kLoadImage = kRowsPerLoad * 2 * KvpCfg::D;   // ... and their bytes in a bf16 image
    static_assert(kLoads * kRowsPerLoad == kKvBlk && 8 <= kPagedMinPage && kPagedMinPage % 8 == 0, "eight rows of a load lie in one 16-row group");
    static_assert(KvpCfg::D == 128, "a row is eight 16-byte chunks of e4m3");
};

// fetch_pages / pages_landed of fa_kv_decode_core.h for the two loads of a wave: rows row0 and row0 + kRowsPerLoad of the block, clamped to
// kend - 1 BEFORE the lookup (only called with kend >= 1)
template <bool WINDOW = false>
__device__ __forceinline__ void kvp8_fetch_pages(cst_i32_t* tbl, int page_shift, int row0, int kend, int (&e)[Kvp8Map::kLoads], int lo = 0)
{
#pragma unroll
    for (int i = 0; i < Kvp8Map::kLoads; ++i) {
        int row = min(row0 + i * Kvp8Map::kRowsPerLoad, kend - 1);
        if constexpr (WINDOW) row = max(row, lo);
        int idx = __builtin_amdgcn_readfirstlane(row) >> page_shift;
        asm volatile("" : "+s"(idx));
        e[i] = tbl[idx];
    }
}
__device__ __forceinline__ void kvp8_pages_landed(int (&e)[Kvp8Map::kLoads], int64_t page_stride, int64_t (&pb)[Kvp8Map::kLoads])
{
#pragma unroll
    for (int i = 0; i < Kvp8Map::kLoads; ++i) asm volatile("" : "+s"(e[i]));
#pragma unroll
    for (int i = 0; i < Kvp8Map::kLoads; ++i) pb[i] = (int64_t)e[i] * page_stride;
}

__device__ __forceinline__ bf16x8 lds_read_b128(unsigned addr)
{
    bf16x8 v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr) : "memory");
    return v;
}
// all but the N most recent LDS reads have landed (they return in order; a table entry in flight on the same counter only makes the wait
// stricter), and nothing the compiler schedules may use x[] before this point
template <int N, typename T, int K>
__device__ __forceinline__ void lds_landed_but(T (&x)[K])
{
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
#pragma unroll
    for (int i = 0; i < K; ++i) asm volatile("" : "+v"(x[i]));
}

template <bool CAUSAL, bool OUT_F32, bool PAGED, bool FP8 = false, typename Params = KvpParams, bool WINDOW = false>
__device__ __forceinline__ void kvp_prefill(const Params& wp, int window_left = 0)
{
    using C = KvpCfg;
    using elem_t = std::conditional_t<FP8, uint8_t, __bf16>;   // FP8: one byte per element, so every offset of the cache is in bytes
    constexpr int D = C::D, KS = C::KS, DB = C::DB, NB = C::NB, NP = FP8 ? Kvp8Map::kLoads : kPagedBlockPages;
    __shared__ __attribute__((aligned(1024))) char smem[2 * C::kStage];

    const PagedParams& pp = wp.pp;
    const KvParams& p = pp.kv;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lq = lane & 31, hi = lane >> 5;
    const int M = p.m_rows, nq = p.nq;

    // ---- the workgroup's tile: slab fastest (the XCDs take workgroups round robin: a slab's tiles meet in one L2 where bh_kv is a multiple
    // of 8), tiles in the order u = 0, 1, ... with the heaviest causal tile first ----
    const int slab = blockIdx.x % p.bh_kv, u = blockIdx.x / p.bh_kv;
    int tile = u;
    if (CAUSAL) {
        tile = wp.tiles - 1 - u;
        if (nq % kKvpRowTile == 0) {   // tiles do not straddle heads: the last tile of every head, then the one before it, ...
            const int per_head = nq / kKvpRowTile, group = M / nq;
            tile = (u % group) * per_head + per_head - 1 - u / group;
        }
    }
    int heads_kv = 1;
    if constexpr (PAGED) heads_kv = pp.heads_kv;
    const int seq = slab / heads_kv, head = slab % heads_kv;
    int len = p.nk;
    if (p.kv_lens != nullptr) len = min(max(p.kv_lens[seq], 0), p.nk);
    const int diag = len - nq;
    // the keys a range of packed rows reads: [0, end), bounded by the range's widest row (0: no row of the slab in it)
    auto keys_of = [&](int r0, int rows) {
        if (r0 >= M) return 0;
        const int rl = min(r0 + rows - 1, M - 1);
        int end = len;
        if (CAUSAL) end = min(end, diag + ((r0 / nq != rl / nq) ? nq - 1 : rl % nq) + 1);
        return max(end, 0);
    };
    const int row0 = tile * kKvpRowTile, wrow0 = row0 + wave * (NB * kKvRowTile);
    const int kend = keys_of(row0, kKvpRowTile);
    const int wend = __builtin_amdgcn_readfirstlane(keys_of(wrow0, NB * kKvRowTile));   // this wave's rows see nothing at or beyond it
    const int nblk = (kend + kKvBlk - 1) / kKvBlk;
    // WINDOW: the first key a range of packed rows sees, that of its lowest row (i = 0 where the range straddles a head, as keys_of has
    // i = nq - 1 there).  lo is the tile's -- kend > lo wherever kend >= 1: the widest row reaches beyond the lowest row's first key -- and
    // every row that is loaded or looked up is clamped to it from below; the walk starts at lo's block, jbeg; wbeg is the wave's.
    int lo = 0, jbeg = 0, wbeg = 0;
    if constexpr (WINDOW) {
        auto first_key_of = [&](int r0, int rows) {
            const int rl = min(r0 + rows - 1, M - 1);
            return max(diag + ((r0 / nq != rl / nq) ? 0 : r0 % nq) - window_left, 0);
        };
        lo = first_key_of(row0, kKvpRowTile);
        jbeg = lo / kKvBlk;
        wbeg = __builtin_amdgcn_readfirstlane(first_key_of(wrow0, NB * kKvRowTile));   // read only where wend > 0, i.e. wrow0 < M
    }

    // ---- Q, the masks ----
    bf16x8 qf[NB][KS];
    int lim[NB], lo_row[NB];
    bool row_ok[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int r0 = wrow0 + nb * kKvRowTile;
        row_ok[nb] = r0 + lq < M;
        lim[nb] = kend - 1;
        if (CAUSAL) lim[nb] = min(lim[nb], diag + (r0 + lq) % nq);
        // WINDOW: the first key this lane's row sees.  CAUSAL, it is lim - window_left and is formed from lim in every step (a row of the
        // slab has i <= the tile's imax, so its lim is diag + i unclipped); otherwise it is held -- FP8, whose vector half is full, in the
        // accumulation half (q_in_registers)
        lo_row[nb] = 0;
        if constexpr (WINDOW && !CAUSAL) lo_row[nb] = diag + (r0 + lq) % nq - window_left;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[nb][ks] = kv_q_fragment<D>(p.q, (int64_t)slab * M + min(r0, M - 1), row_ok[nb], lq, hi, ks);
    }
    auto q_in_registers = [&]() {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if (nb == 0) asm volatile("" : "+v"(qf[nb][ks]));
                else asm volatile("" : "+a"(qf[nb][ks]));
            }
        if constexpr (WINDOW && FP8)   // the lane's bound: lim where both come from it, lo_row beside a uniform lim
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) asm volatile("" : "+a"(CAUSAL ? lim[nb] : lo_row[nb]));
    };
    q_in_registers();
    bf16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;

    const elem_t *kg, *vg;
    cst_i32_t* tbl = nullptr;
    int page_mask = 0;
    unsigned row_stride = 0;
    if constexpr (PAGED) {
        kg = (const elem_t*)p.k + (int64_t)head * pp.head_stride;
        vg = (const elem_t*)p.v + (int64_t)head * pp.head_stride;
        tbl = (cst_i32_t*)(pp.table + (int64_t)seq * pp.max_pages);
        page_mask = (1 << pp.page_shift) - 1;
        row_stride = (unsigned)pp.row_stride;
    } else {
        kg = (const elem_t*)p.k + (int64_t)slab * p.kv_slab_stride;
        vg = (const elem_t*)p.v + (int64_t)slab * p.kv_slab_stride;
    }

    // ---- this lane's part of a piece: its row within the piece's 16-row group and its column (issue_k_tile / issue_v_tile of
    // fa_bf16_common.h for piece wave + 4 i: the swizzle of a K row depends on the row's low four bits, which i does not touch) ----
    const int k_row = 4 * wave + (lane >> 4), k_col = ((lane & 15) ^ (k_row & 15)) * 8;
    const int v_row = 4 * wave + ((lane & 7) >> 1), v_col = (lane >> 3) * 16 + (lane & 1) * 8;
    auto issue = [&](int kv0, const int64_t(&pb)[NP], char* stage) {
        if constexpr (!FP8)
#pragma unroll
        for (int i = 0; i < C::kPieces; ++i) {
            int kr = min(kv0 + 16 * i + k_row, kend - 1), vr = min(kv0 + 16 * i + v_row, kend - 1);
            if constexpr (WINDOW) kr = max(kr, lo), vr = max(vr, lo);   // the walk's first block may begin below lo
            const char *ks, *vs;
            if constexpr (PAGED) {
                ks = (const char*)(kg + pb[i]) + ((unsigned)(kr & page_mask) * row_stride + k_col) * 2u;
                vs = (const char*)(vg + pb[i]) + ((unsigned)(vr & page_mask) * row_stride + v_col) * 2u;
            } else {
                ks = (const char*)kg + ((unsigned)kr * (unsigned)(2 * D) + k_col * 2);
                vs = (const char*)vg + ((unsigned)vr * (unsigned)(2 * D) + v_col * 2);
            }
            __builtin_amdgcn_global_load_lds((gbl_cvoid_t*)ks, (lds_void_t*)(stage + (wave + kKvWaves * i) * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gbl_cvoid_t*)vs, (lds_void_t*)(stage + C::kImage + (wave + kKvWaves * i) * 1024), 16, 0, 0);
        }
    };

    // ---- FP8: the block through registers (Kvp8Map).  raw[i] is K's load i, raw[kLoads + i] V's: ordinary loads, counted in vmcnt by hipcc.
    // The lane's coordinates are derived from its number where they are used, behind an empty statement, not held through the loop ----
    constexpr int NL = Kvp8Map::kLoads;
    int lane_v = lane;
    auto load_raw = [&](int kv0, const int64_t(&pb)[NP], u32x4(&raw)[2 * NL]) {
        if constexpr (FP8) {
            asm volatile("" : "+v"(lane_v));
            const int k_key = 8 * wave + (lane_v >> 3), k_chunk = lane_v & 7;
            const int v_key = 8 * wave + 4 * (lane_v >> 5) + ((lane_v >> 1) & 3), v_chunk = (lane_v & 1) + 2 * ((lane_v >> 3) & 3);
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                int kr = min(kv0 + i * Kvp8Map::kRowsPerLoad + k_key, kend - 1), vr = min(kv0 + i * Kvp8Map::kRowsPerLoad + v_key, kend - 1);
                if constexpr (WINDOW) kr = max(kr, lo), vr = max(vr, lo);
                const uint8_t *ks, *vs;
                if constexpr (PAGED) {
                    ks = kg + pb[i] + ((unsigned)(kr & page_mask) * row_stride + k_chunk * 16);
                    vs = vg + pb[i] + ((unsigned)(vr & page_mask) * row_stride + v_chunk * 16);
                } else {
                    ks = kg + ((unsigned)kr * (unsigned)D + k_chunk * 16);
                    vs = vg + ((unsigned)vr * (unsigned)D + v_chunk * 16);
                }
                raw[i] = *(const u32x4*)ks;
                raw[NL + i] = *(const u32x4*)vs;
            }
            asm volatile("" ::: "memory");   // the loads stay in front of the block's compute: they are what is in flight under it
        }
    };
    // ... converted exactly and written into the two bf16 images of `stage` (an LDS byte offset), two ds_write_b128 per load
    auto convert_store = [&](const u32x4(&raw)[2 * NL], int stage) {
        if constexpr (FP8) {
            asm volatile("" : "+v"(lane_v));
            const int k_key = 8 * wave + (lane_v >> 3), v_key4 = 2 * wave + (lane_v >> 5), v_chunk = (lane_v & 1) + 2 * ((lane_v >> 3) & 3);
            const int k_wr = stage + k_key * (2 * D) + (((2 * (lane_v & 7)) ^ (k_key & 15)) << 4);
            const int v_wr = stage + C::kImage + v_key4 * 1024 + v_chunk * 128 + ((lane_v >> 1) & 3) * 32;
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                *(bf16x8*)(smem + i * Kvp8Map::kLoadImage + k_wr) = cvt_fp8x8(raw[i][0], raw[i][1]);
                *(bf16x8*)(smem + i * Kvp8Map::kLoadImage + (k_wr ^ 16)) = cvt_fp8x8(raw[i][2], raw[i][3]);
                *(bf16x8*)(smem + i * Kvp8Map::kLoadImage + v_wr) = cvt_fp8x8(raw[NL + i][0], raw[NL + i][1]);
                *(bf16x8*)(smem + i * Kvp8Map::kLoadImage + v_wr + 16) = cvt_fp8x8(raw[NL + i][2], raw[NL + i][3]);
            }
        }
    };
    // my stores have landed (and, PAGED, the entries in flight: they are a block old)
    auto stores_landed = [&]() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); };

    // ---- this lane's corners of the fragments ----
    // K: key kb * 32 + lq of the image, columns 16 ks + 8 hi .. + 8 = slot 2 ks + hi, swizzled by the row's low four bits
    const unsigned k_lane_off = lq * (2 * D), k_g = lq & 15;
    // V^T: [key/4][col/16][4][16] sub-tiles, keys permuted like the scores (fa_kv_decode16_body.h)
    const int li = lane & 15;
    const unsigned v_lane_off = C::kImage + (hi * (D / 16) + ((lane >> 4) & 1)) * 128 + (li >> 2) * 32 + (li & 3) * 8;
    const float c = p.scale_log2e;

    f32x16 o[NB][DB], lacc[NB];
    float m[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        m[nb] = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) lacc[nb][r] = 0.0f;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[nb][db][r] = 0.0f;
    }

    // the V^T fragments of 16 keys (kb, t) for all four column blocks of O
    auto read_v = [&](unsigned v_addr, int f, s16x4(&vv)[2 * DB]) {
#pragma unroll
        for (int db = 0; db < DB; ++db) {
            vv[2 * db] = lds_read_tr16(v_addr + (((f >> 1) * 8 + 4 * (f & 1) + 0) * (D / 16) + 2 * db) * 128);
            vv[2 * db + 1] = lds_read_tr16(v_addr + (((f >> 1) * 8 + 4 * (f & 1) + 2) * (D / 16) + 2 * db) * 128);
        }
    };

    // One 64-key block, as two halves of 32 keys (one MFMA row block of S^T each, with the 32-key softmax step of fa_kv256_decode_loop.h): the
    // scores and P of both row blocks are 32 + 32 registers live at a time instead of 64 + 64, which is what lets Q stay in registers.
    auto compute = [&](int kv0, unsigned stage) __attribute__((always_inline)) {
        const unsigned k_addr = stage + k_lane_off, v_addr = stage + v_lane_off;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h == 1 && kv0 + 32 >= wend) break;   // the wave's rows see nothing of the second half
            if constexpr (WINDOW)
                if (h == 0 && kv0 + 32 <= wbeg) continue;   // ... or, below their window, of the first
            // ---- S^T = K Q^T ----
            bf16x8 kf[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) kf[ks] = lds_read_b128(k_addr + h * 32 * (2 * D) + (((2 * ks + hi) ^ k_g) * 16));
            f32x16 s[NB];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) s[nb][r] = 0.0f;
            lds_landed_but<0>(kf);
            s16x4 va[2 * DB], vb[2 * DB];
            read_v(v_addr, 2 * h, va);   // lands under the products and the softmax
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) s[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[nb][ks], s[nb], 0, 0, 0);

            // ---- online softmax, per row block ----
            bf16x8 ph[NB][2], pl[NB][2];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const KvRescale rs = kv256_mask_and_max<WINDOW>(s[nb], lim[nb] - kv0 - 32 * h - 4 * hi, c, m[nb],
                                                                   (CAUSAL ? lim[nb] - window_left : lo_row[nb]) - kv0 - 32 * h - 4 * hi);
                if (__builtin_amdgcn_ballot_w64(rs.alpha != 1.0f) != 0) {   // some row's maximum moved
#pragma unroll
                    for (int db = 0; db < DB; ++db)
#pragma unroll
                        for (int r = 0; r < 16; ++r) o[nb][db][r] *= rs.alpha;
#pragma unroll
                    for (int r = 0; r < 16; ++r) lacc[nb][r] *= rs.alpha;
                }
                kv256_p_terms(s[nb], rs.m_use, ph[nb], pl[nb]);
            }

            // ---- O^T += V^T P^T, 16 keys at a time: the second 16 keys' fragments in flight under the first's products ----
            auto pv = [&](int t, const s16x4(&vv)[2 * DB]) {
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    const bf16x8 vf = __builtin_bit_cast(bf16x8, __builtin_shufflevector(vv[2 * db], vv[2 * db + 1], 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) {
                        o[nb][db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, ph[nb][t], o[nb][db], 0, 0, 0);
                        o[nb][db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pl[nb][t], o[nb][db], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    lacc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, ph[nb][t], lacc[nb], 0, 0, 0);
                    lacc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, pl[nb][t], lacc[nb], 0, 0, 0);
                }
            };
            read_v(v_addr, 2 * h + 1, vb);
            lds_landed_but<2 * DB>(va);
            pv(0, va);
            lds_landed_but<0>(vb);
            pv(1, vb);
            q_in_registers();
        }
    };

    // ---- the walk ----
    int64_t pg[NP];
    int ent[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) pg[i] = 0, ent[i] = 0;
    // the entries of the block at kv0 (FP8: of this wave's two loads of it), and the point up to which they must have arrived
    auto fetch = [&](int kv0, int(&e)[NP]) {
        if constexpr (FP8) kvp8_fetch_pages<WINDOW>(tbl, pp.page_shift, kv0 + 8 * wave, kend, e, lo);
        else fetch_pages<WINDOW>(tbl, pp.page_shift, kv0, kend, e, lo);
    };
    auto landed = [&](int(&e)[NP]) {
        if constexpr (FP8) kvp8_pages_landed(e, pp.page_stride, pg);
        else pages_landed(e, pp.page_stride, pg);
    };
    u32x4 raw[2 * NL];   // FP8: the bytes of the next block, from the top of a block to its end
    if (nblk > 0) {   // kend >= 1 from here on: every row (and, PAGED, every table index) is that of a key below len
        if constexpr (PAGED) {
            int e0[NP];
            fetch(jbeg * kKvBlk, e0);
            fetch((jbeg + 1) * kKvBlk, ent);
            landed(e0);
        }
        if constexpr (FP8) {
            load_raw(jbeg * kKvBlk, pg, raw);
            convert_store(raw, 0);
        } else {
            issue(jbeg * kKvBlk, pg, smem);
        }
    }
    const unsigned lds0 = (unsigned)(size_t)(lds_void_t*)smem;
    for (int j = jbeg; j < nblk; ++j) {   // WINDOW: from the block of the tile's lowest key on (jbeg = 0 otherwise)
        if constexpr (FP8) stores_landed();   // my part of block j
        else wait_lds_dma();                  // my pieces of block j
        __builtin_amdgcn_s_barrier();    // everybody's; and everybody has read block j - 1
        asm volatile("" ::: "memory");
        const int par = (j - jbeg) & 1;   // the stages alternate from the walk's first block on
        if (j + 1 < nblk) {
            if constexpr (PAGED) {
                landed(ent);                        // block j + 1: fetched a block ago
                fetch((j + 2) * kKvBlk, ent);       // block j + 2
            }
            if constexpr (FP8) load_raw((j + 1) * kKvBlk, pg, raw);
            else issue((j + 1) * kKvBlk, pg, smem + (par ^ 1) * C::kStage);
        }
        bool mine = j * kKvBlk < wend;
        if constexpr (WINDOW) mine = mine && (j + 1) * kKvBlk > wbeg;   // ... nor is the block wholly below the wave's window
        if (mine) compute(j * kKvBlk, lds0 + par * C::kStage);
        if constexpr (FP8)   // block j + 1 into the other stage, which everybody left before this block's barrier
            if (j + 1 < nblk) convert_store(raw, (par ^ 1) * C::kStage);
    }
    mfma_drain();   // the loop exit is a branch: the last matrix instructions may still be in flight

    // ---- epilogue: every wave stores its own rows.  Lane (lq, hi) holds columns 32 db + 8 g + 4 hi .. + 4 of row lq in o[.][db][4 g ..] ----
    // (WINDOW over an fp8 cache: the lane's coordinates are derived from its number again, behind an empty statement, as in
    // fa_kvp256_prefill_loop.h -- held through the loop beside the raw bytes and the lower bound they would not fit)
    int lq_e = lq, hi_e = hi;
    if constexpr (WINDOW && FP8) {
        asm volatile("" : "+v"(lane_v));
        lq_e = lane_v & 31, hi_e = lane_v >> 5;
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        if ((WINDOW && FP8) ? wrow0 + nb * kKvRowTile + lq_e >= M : !row_ok[nb]) continue;
        const float l = lacc[nb][0];
        const bool none = !(l > 0.0f);   // no visible key: O = 0, LSE = -inf
        const int64_t prow = (int64_t)slab * M + wrow0 + nb * kKvRowTile + lq_e;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 acc;
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = none ? 0.0f : o[nb][db][4 * g + e] / l;
                if constexpr (FP8)   // once, behind the quotient: a constant V comes out as exactly v_scale x it
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] *= wp.v_scale;
                const int col = db * 32 + 8 * g + 4 * hi_e;
                if (OUT_F32) {
                    *(f32x4*)((float*)p.o + prow * D + col) = acc;
                } else {
                    bf16x4 r;
#pragma unroll
                    for (int e = 0; e < 4; ++e) r[e] = (__bf16)acc[e];
                    *(bf16x4*)((__bf16*)p.o + prow * D + col) = r;
                }
            }
        if (hi_e == 0 && p.lse != nullptr) p.lse[prow] = none ? -INFINITY : (m[nb] + __builtin_amdgcn_logf(l)) * kLn2;
    }
}

}  // namespace fa
