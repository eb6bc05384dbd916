// fa_kvp256_prefill_loop.h -- chunked prefill over a bf16 cache at head dim 256, contiguous or paged: the kernel of libflashattn_amd_kvp256.so
// (fa_kvp256_prefill.hip instantiates it eight times).  The d = 256 twin of fa_kvp_prefill_loop.h: the same packed rows, masks, arithmetic
// and one-barrier protocol, with a work split, an LDS map and a register plan of its own.  No counterpart in the reference.
// With WINDOW = true it is the d = 256 kernel of libflashattn_amd_kvpw.so (fa_kvpw256_prefill.hip; "WINDOW" in fa_kvp_prefill_loop.h says what
// changes: the same here).  Out of scope: fp8 caches, a key split for tiny grids, routing from fa_kv256_forward.
//
// Work split.  A workgroup of four waves owns (K/V slab, 128-row tile of the slab's packed rows); wave w takes rows 32 w .. 32 w + 31 of the
// tile as ONE 32-row MFMA column block (the d = 128 loop: two; O for two would be 2 x 128 registers, the whole accumulation half).  All four
// waves walk the SAME 64-key blocks, from key 0 to the tile's kend = min(len, diag + imax + 1): no key split, no workspace, no merge.  Causal
// tiles are launched heaviest first.
//
// LDS: two stages of one 64-key block, 128 KiB static, one workgroup per CU (the budget class of fa_kv256_decode_loop.h).  A stage is
//   K  32 KiB: row-major, 64 keys at a 512-byte pitch = 32 slots of 16 bytes, slot s of row r kept at s ^ (r & 15): the row's low FOUR bits
//      feed the low four bits of the five-bit slot.  The pitch is two times the 256 bytes the 64 banks span, so every row starts at bank 0 and
//      the bank group of a slot is its low four bits alone: the XOR of fa_bf16_common.h carries over on those bits, and bit 4 of the slot
//      (columns 128 and up) needs none.  A ds_read_b128 serves 16 lanes per pass; lanes of one pass read 16 consecutive keys at one logical
//      slot, so their low row bits are the sixteen values and they land in sixteen different bank groups.  The LDS-DMA writes of a piece are
//      1 KiB linear in LDS whatever the swizzle (lane l writes bytes 16 l .. + 15 of the piece: two whole rows); the swizzle is in which
//      16 global bytes of its row a lane fetches, all inside one 512-byte row: they meet in no bank either.
//   V  32 KiB: the [key/4][col/16][4][16] sub-tile image of fa_kv256_decode_loop.h (a 4-key group is sixteen 128-byte sub-tiles), read with
//      ds_read_b64_tr_b16.
// Two stages of 64 keys, not of 32: half the barriers for the same bytes, and the 128 KiB are there (one workgroup per CU either way, since a
// wave holds the whole SIMD's registers).
//
// Data movement: LDS-DMA (global_load_lds, 16 bytes per lane).  A block is 32 + 32 pieces of 1 KiB; a wave brings in eight of each, so 16
// loads per wave are outstanding at most (vmcnt has 6 bits).  One barrier per block, the protocol of fa_kvp_prefill_loop.h:
//     wait for my pieces of block j;  barrier;  enqueue block j + 1 into the other stage;  compute block j
// Piece i of a wave (i = 0 .. 7) is K rows 16 (i / 2) + 4 w + 2 (i % 2) .. + 1 and V rows 16 (i / 2) + 4 w .. + 3 (column half i % 2) of the
// block: inside the block's 16-row group i / 2, so its table entry is a compile-time index (KvpCfg256's static_assert).
// LDS reads are inline asm with hand-counted lgkmcnt (hipcc puts "wait for EVERY LDS-DMA in flight" in front of each LDS read it can see).
// lgkmcnt has four bits, so the V^T fragments are read in chunks of eight (four column blocks of O for 16 keys), two chunks in flight: the
// next chunk is issued under the products of the current one, and the K fragments of the block's second 32 keys under the last products of
// the first.  Compile-time parts of an address ride in the instruction's offset field.
//
// Registers (one wave per SIMD, 512; no scratch: the figures of the code object are in docs/kv_prefill_d256.md).  The accumulation half
// holds O (8 x 16), the row sum (16), the scores of a 32-key step (16) and Q (64, pinned there: only the matrix pipe reads it); the other half
// the K fragments of a step (64), P hi + lo (16) and the V^T chunks in flight.
//
// Arithmetic: the contract of the KV libraries, with the 32-key softmax step of fa_kv256_decode_loop.h (kv256_mask_and_max<false>,
// kv256_p_terms).  S^T = K Q^T on v_mfma_f32_32x32x16_bf16, one bf16 product; P = bf16 hi + bf16 lo; the row sum on the matrix pipe against
// all-ones in the instruction sequence of every O column.  O and the row sum are rescaled only in a step where some row's maximum moved (a
// wave-uniform branch; alpha = 1 elsewhere, so the bits are those of the unconditional product).
//
// Edges, as in fa_kvp_prefill_loop.h: rows past M are computed on zeros and never stored; i = r % nq, so tiles and row blocks may straddle
// heads; len = min(max(kv_lens[seq], 0), nk) is read here; loads of rows at or beyond kend are redirected to row kend - 1 BEFORE the table
// lookup; a tile without a visible key touches neither K, V nor the table and stores 0 / -inf.  A wave whose rows see nothing of a block, or
// of its second 32 keys, skips the matrix work, but still brings its pieces in and meets the barrier.
// Paged: the address rule of fa_kv_decode_core.h, entries read through the constant address space one block ahead of the DMA that uses them;
// a 64-bit uniform base plus a 32-bit offset per lane, under the host checks of fa_kv_host.h.
#pragma once
#include "fa_kvp_prefill_loop.h"   // lds_landed_but; through it fa_kv256_decode_loop.h (the softmax step) and fa_kv_decode_core.h
#include "fa_kvp256.h"

#include <utility>

namespace fa {

struct Kvp256Cfg {
    static constexpr int D = kKvp256HeadDim, KS = D / 16, DB = D / 32;
    static constexpr int kRowBytes = 2 * D;                       // the K image's pitch
    static constexpr int kImage = kKvBlk * kRowBytes;             // bytes of one K or V image (64 keys)
    static constexpr int kStage = 2 * kImage;                     // K, then V
    static constexpr int kPieces = kImage / 1024 / kKvWaves;      // 1 KiB DMA pieces per wave and image
    static constexpr int kVChunk = 4;                             // column blocks of O whose V^T fragments are read together
    static constexpr int kKeyGroup = 4 * kRowBytes;               // bytes of four keys in the V image
    static_assert(kKvp256RowTile == kKvWaves * kKvRowTile, "four waves of one row block");
    static_assert(kPieces == 2 * kPagedBlockPages && 2 * (1024 / kRowBytes) * kKvWaves == kPagedMinPage, "pieces 2 g and 2 g + 1 of a wave lie in the block's 16-row group g");
    static_assert(2 * kPieces <= 63, "vmcnt holds 6 bits");
    static_assert(2 * kVChunk <= 15, "lgkmcnt holds 4 bits");
    static_assert(2 * kStage <= 160 * 1024, "two stages in the LDS of a CU");
    static_assert(kImage + 3 * kKeyGroup <= 65536, "the 16-bit offset field of a V^T read");
};

template <int OFF>
__device__ __forceinline__ bf16x8 lds_read_b128_at(unsigned addr)
{
    bf16x8 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}
template <int OFF>
__device__ __forceinline__ s16x4 lds_read_tr16_at(unsigned addr)
{
    s16x4 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}

// the K fragments of 32 keys: ka[j] is this lane's address of logical slot 2 j + hi of its key (swizzled); slots 16 and up are 256 bytes on
template <int... KSI>
__device__ __forceinline__ void kvp256_read_k(const unsigned (&ka)[8], bf16x8 (&kf)[Kvp256Cfg::KS], std::integer_sequence<int, KSI...>)
{
    ((kf[KSI] = lds_read_b128_at<(KSI >> 3) * 256>(ka[KSI & 7])), ...);
}
// the V^T fragments of 16 keys for column blocks DB0 .. DB0 + 3 of O: key groups 0 and 2 from va (the caller adds 4 t + hi key groups)
template <int DB0, int... I>
__device__ __forceinline__ void kvp256_read_v(unsigned va, s16x4 (&vv)[2 * Kvp256Cfg::kVChunk], std::integer_sequence<int, I...>)
{
    using C = Kvp256Cfg;
    ((vv[2 * I] = lds_read_tr16_at<C::kImage + 2 * (DB0 + I) * 128>(va), vv[2 * I + 1] = lds_read_tr16_at<C::kImage + 2 * C::kKeyGroup + 2 * (DB0 + I) * 128>(va)), ...);
}

template <bool CAUSAL, bool OUT_F32, bool PAGED, bool WINDOW = false>
__device__ __forceinline__ void kvp256_prefill(const Kvp256Params& wp, int window_left = 0)
{
    using C = Kvp256Cfg;
    constexpr int D = C::D, KS = C::KS, DB = C::DB, NP = kPagedBlockPages, VC = C::kVChunk;
    __shared__ __attribute__((aligned(1024))) char smem[2 * C::kStage];

    const PagedParams& pp = wp.pp;
    const KvParams& p = pp.kv;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lq = lane & 31, hi = lane >> 5;
    const int M = p.m_rows, nq = p.nq;

    // ---- the workgroup's tile: slab fastest, tiles in the order u = 0, 1, ... with the heaviest causal tile first ----
    const int slab = blockIdx.x % p.bh_kv, u = blockIdx.x / p.bh_kv;
    int tile = u;
    if (CAUSAL) {
        tile = wp.tiles - 1 - u;
        if (nq % kKvp256RowTile == 0) {   // tiles do not straddle heads: the last tile of every head, then the one before it, ...
            const int per_head = nq / kKvp256RowTile, group = M / nq;
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
    const int row0 = tile * kKvp256RowTile, wrow0 = row0 + wave * kKvRowTile;
    const int kend = keys_of(row0, kKvp256RowTile);
    const int wend = __builtin_amdgcn_readfirstlane(keys_of(wrow0, kKvRowTile));   // this wave's rows see nothing at or beyond it
    const int nblk = (kend + kKvBlk - 1) / kKvBlk;
    // WINDOW, as in fa_kvp_prefill_loop.h: the tile's lowest visible key lo (the lower clamp of every row loaded or looked up; kend > lo
    // wherever kend >= 1), its block jbeg, where the walk starts, and the wave's lowest visible key wbeg
    int lo = 0, jbeg = 0, wbeg = 0;
    if constexpr (WINDOW) {
        auto first_key_of = [&](int r0, int rows) {
            const int rl = min(r0 + rows - 1, M - 1);
            return max(diag + ((r0 / nq != rl / nq) ? 0 : r0 % nq) - window_left, 0);
        };
        lo = first_key_of(row0, kKvp256RowTile);
        jbeg = lo / kKvBlk;
        wbeg = __builtin_amdgcn_readfirstlane(first_key_of(wrow0, kKvRowTile));   // read only where wend > 0, i.e. wrow0 < M
    }

    // ---- Q, the mask ----
    const bool row_ok = wrow0 + lq < M;
    int lim = kend - 1, lo_row = 0;
    if (CAUSAL) lim = min(lim, diag + (wrow0 + lq) % nq);
    if constexpr (WINDOW) lo_row = diag + (wrow0 + lq) % nq - window_left;   // the first key this lane's row sees
    bf16x8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = kv_q_fragment<D>(p.q, (int64_t)slab * M + min(wrow0, M - 1), row_ok, lq, hi, ks);
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
        kg = (const __bf16*)p.k + (int64_t)head * pp.head_stride;
        vg = (const __bf16*)p.v + (int64_t)head * pp.head_stride;
        tbl = (cst_i32_t*)(pp.table + (int64_t)seq * pp.max_pages);
        page_mask = (1 << pp.page_shift) - 1;
        row_stride = (unsigned)pp.row_stride;
    } else {
        kg = (const __bf16*)p.k + (int64_t)slab * p.kv_slab_stride;
        vg = (const __bf16*)p.v + (int64_t)slab * p.kv_slab_stride;
    }

    // ---- this lane's part of a piece.  K piece 8 g + 2 wave + b (g = i / 2, b = i % 2) is rows 2 * piece .. + 1 of the image: lane l writes
    // physical slot l & 31 of row 16 g + 4 wave + 2 b + (l >> 5), so it fetches logical slot (l & 31) ^ (row & 15); b flips bit 1 of the row.
    // V piece 8 g + 2 wave + b is column half b of keys 16 g + 4 wave .. + 3 (issue_v of fa_kv256_decode_loop.h) ----
    const int k_row = 4 * wave + (lane >> 5), k_colb = ((lane & 31) ^ (k_row & 15)) * 16;
    const int v_row = 4 * wave + ((lane & 7) >> 1), v_col = (lane >> 3) * 16 + (lane & 1) * 8;
    auto issue = [&](int kv0, const int64_t(&pb)[NP], char* stage) {
#pragma unroll
        for (int i = 0; i < C::kPieces; ++i) {
            constexpr int kHalf = D / 2;
            const int g = i >> 1, b = i & 1;
            int kr = min(kv0 + 16 * g + 2 * b + k_row, kend - 1), vr = min(kv0 + 16 * g + v_row, kend - 1);
            if constexpr (WINDOW) kr = max(kr, lo), vr = max(vr, lo);   // the walk's first block may begin below lo
            const unsigned kc = (unsigned)(k_colb ^ (32 * b)), vc = (unsigned)(b * kHalf + v_col) * 2u;
            const char *ks, *vs;
            if constexpr (PAGED) {
                ks = (const char*)(kg + pb[g]) + ((unsigned)(kr & page_mask) * row_stride * 2u + kc);
                vs = (const char*)(vg + pb[g]) + ((unsigned)(vr & page_mask) * row_stride * 2u + vc);
            } else {
                ks = (const char*)kg + ((unsigned)kr * (unsigned)C::kRowBytes + kc);
                vs = (const char*)vg + ((unsigned)vr * (unsigned)C::kRowBytes + vc);
            }
            const int piece = 8 * g + 2 * wave + b;
            __builtin_amdgcn_global_load_lds((gbl_cvoid_t*)ks, (lds_void_t*)(stage + piece * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gbl_cvoid_t*)vs, (lds_void_t*)(stage + C::kImage + piece * 1024), 16, 0, 0);
        }
    };

    // ---- this lane's corners of the fragments ----
    // K: key 32 h + lq of the image, columns 16 ks + 8 hi .. + 8 = logical slot 2 ks + hi = 16 (ks >> 3) + (2 (ks & 7) + hi)
    // ((2 j + hi) ^ g) * 16 = ((32 j) ^ k_swz) + the lane's constant part, g = lq & 15: two registers through the loop, not eight
    const unsigned k_lane_off = lq * C::kRowBytes + ((hi ^ (lq & 1)) * 16), k_swz = (lq & 14) * 16;
    // V^T: [key/4][col/16][4][16] sub-tiles, keys permuted like the scores (fa_kv_decode16_body.h); key group hi of a 16-key step
    const int li = lane & 15;
    const unsigned v_lane_off = hi * C::kKeyGroup + ((lane >> 4) & 1) * 128 + (li >> 2) * 32 + (li & 3) * 8;
    const float c = p.scale_log2e;

    f32x16 o[DB], lacc;
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) lacc[r] = 0.0f;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] = 0.0f;

    constexpr auto kAllKs = std::make_integer_sequence<int, KS>{};
    constexpr auto kChunk = std::make_integer_sequence<int, VC>{};

    // One 64-key block as two steps of 32 keys.  Per step: 16 K reads, 16 products for S^T, the softmax step, and four chunks of V^T
    // fragments (8 reads, 4 column blocks of 16 keys each) against P hi and P lo, two chunks in flight.
    auto compute = [&](int kv0, unsigned stage) __attribute__((always_inline)) {
        unsigned ka[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) ka[j] = stage + k_lane_off + ((32 * j) ^ k_swz);
        const bool second = kv0 + 32 < wend;   // wave-uniform: the wave's rows see something of the second 32 keys
        bool first = true;                     // ... and of the first (WINDOW: not where they lie below the wave's window; `second` holds then)
        if constexpr (WINDOW) {
            first = kv0 + 32 > wbeg;
            if (!first)
#pragma unroll
                for (int j = 0; j < 8; ++j) ka[j] += 32 * C::kRowBytes;
        }
        bf16x8 kf[KS];
        kvp256_read_k(ka, kf, kAllKs);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h == 1 && !second) break;
            if constexpr (WINDOW)
                if (h == 0 && !first) continue;
            // ---- S^T = K Q^T ----
            f32x16 s;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 0.0f;
            lds_landed_but<0>(kf);
            const unsigned va = stage + v_lane_off + h * 8 * C::kKeyGroup;   // the step's first 16 keys; the second 16 are four key groups on
            s16x4 c0[2 * VC], c1[2 * VC], c2[2 * VC], c3[2 * VC];
            kvp256_read_v<0>(va, c0, kChunk);   // land under the products and the softmax
            kvp256_read_v<VC>(va, c1, kChunk);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], s, 0, 0, 0);

            // ---- online softmax ----
            bf16x8 ph[2], pl[2];
            const KvRescale rs = kv256_mask_and_max<WINDOW>(s, lim - kv0 - 32 * h - 4 * hi, c, m, lo_row - kv0 - 32 * h - 4 * hi);
            if (__builtin_amdgcn_ballot_w64(rs.alpha != 1.0f) != 0) {   // some row's maximum moved
#pragma unroll
                for (int db = 0; db < DB; ++db)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[db][r] *= rs.alpha;
#pragma unroll
                for (int r = 0; r < 16; ++r) lacc[r] *= rs.alpha;
            }
            kv256_p_terms(s, rs.m_use, ph, pl);

            // ---- O^T += V^T P^T: chunk (t, d0) is column blocks d0 .. d0 + 3 against the 16 keys t ----
            auto pv = [&](int t, int d0, const s16x4(&vv)[2 * VC]) {
#pragma unroll
                for (int i = 0; i < VC; ++i) {
                    const bf16x8 vf = __builtin_bit_cast(bf16x8, __builtin_shufflevector(vv[2 * i], vv[2 * i + 1], 0, 1, 2, 3, 4, 5, 6, 7));
                    o[d0 + i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, ph[t], o[d0 + i], 0, 0, 0);
                    o[d0 + i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pl[t], o[d0 + i], 0, 0, 0);
                }
                if (d0 + VC == DB) {
                    lacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, ph[t], lacc, 0, 0, 0);
                    lacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, pl[t], lacc, 0, 0, 0);
                }
            };
            lds_landed_but<2 * VC>(c0);
            pv(0, 0, c0);
            kvp256_read_v<0>(va + 4 * C::kKeyGroup, c2, kChunk);
            lds_landed_but<2 * VC>(c1);
            pv(0, VC, c1);
            kvp256_read_v<VC>(va + 4 * C::kKeyGroup, c3, kChunk);
            lds_landed_but<2 * VC>(c2);
            pv(1, 0, c2);
            lds_landed_but<0>(c3);
            if (h == 0 && second) {   // the second step's K fragments land under the first step's last products
#pragma unroll
                for (int j = 0; j < 8; ++j) ka[j] += 32 * C::kRowBytes;
                kvp256_read_k(ka, kf, kAllKs);
            }
            pv(1, VC, c3);
            q_in_acc_half();
        }
    };

    // ---- the walk ----
    int64_t pg[NP];
    int ent[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) pg[i] = 0, ent[i] = 0;
    if (nblk > 0) {   // kend >= 1 from here on: every row (and, PAGED, every table index) is that of a key below len
        if constexpr (PAGED) {
            int e0[NP];
            fetch_pages<WINDOW>(tbl, pp.page_shift, jbeg * kKvBlk, kend, e0, lo);
            fetch_pages<WINDOW>(tbl, pp.page_shift, (jbeg + 1) * kKvBlk, kend, ent, lo);
            pages_landed(e0, pp.page_stride, pg);
        }
        issue(jbeg * kKvBlk, pg, smem);
    }
    const unsigned lds0 = (unsigned)(size_t)(lds_void_t*)smem;
    for (int j = jbeg; j < nblk; ++j) {   // WINDOW: from the block of the tile's lowest key on (jbeg = 0 otherwise)
        wait_lds_dma();                  // my pieces of block j
        __builtin_amdgcn_s_barrier();    // everybody's; and everybody has read block j - 1
        asm volatile("" ::: "memory");
        const int par = (j - jbeg) & 1;   // the stages alternate from the walk's first block on
        if (j + 1 < nblk) {
            if constexpr (PAGED) {
                pages_landed(ent, pp.page_stride, pg);                        // block j + 1: fetched a block ago
                fetch_pages<WINDOW>(tbl, pp.page_shift, (j + 2) * kKvBlk, kend, ent, lo);   // block j + 2
            }
            issue((j + 1) * kKvBlk, pg, smem + (par ^ 1) * C::kStage);
        }
        bool mine = j * kKvBlk < wend;
        if constexpr (WINDOW) mine = mine && (j + 1) * kKvBlk > wbeg;   // ... nor is the block wholly below the wave's window
        if (mine) compute(j * kKvBlk, lds0 + par * C::kStage);
    }
    mfma_drain();   // the loop exit is a branch: the last matrix instructions may still be in flight

    // ---- epilogue: every wave stores its own rows.  Lane (lq, hi) holds columns 32 db + 8 g + 4 hi .. + 4 of row lq in o[db][4 g ..] ----
    // (the lane's coordinates are derived from its number again, behind an empty statement: not held through the loop)
    int lane_e = lane;
    asm volatile("" : "+v"(lane_e));
    const int lq_e = lane_e & 31, hi_e = lane_e >> 5;
    if (wrow0 + lq_e >= M) return;
    const float l = lacc[0];
    const bool none = !(l > 0.0f);   // no visible key: O = 0, LSE = -inf
    const int64_t prow = (int64_t)slab * M + wrow0 + lq_e;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 acc;
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = none ? 0.0f : o[db][4 * g + e] / l;
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
    if (hi_e == 0 && p.lse != nullptr) p.lse[prow] = none ? -INFINITY : (m + __builtin_amdgcn_logf(l)) * kLn2;
}

}  // namespace fa
