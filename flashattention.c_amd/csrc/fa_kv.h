// fa_kv.h -- what the translation units of libflashattn_amd_kv.so share (include/flashattn_amd_kv.h is the boundary): the plan
// of a KV-cache forward, the launch parameters of its kernels and the launchers.  The library is self-contained: it includes
// headers of csrc/ (fa_common.h, fa_bf16_common.h) and links no object of the product library.
#pragma once
#include "fa_common.h"

namespace fa {

constexpr int kKvRowTile = 32;        // packed query rows per workgroup: one 32x32x16 MFMA block column
constexpr int kKvMaxSplits = 64;      // key shares per row tile
constexpr int kKvWaves = 4;
// the two plan constants.  profiles/kv_decode.py sweeps them by building fa_kv_plan.cpp with other values (build.py: build_kv_variant)
// into libraries of its own; docs/kv_decode.md has the table.  256 workgroups = one per CU (a d = 128 workgroup takes 128 KiB of a CU's
// LDS: a second round of workgroups only queues behind the first); 256 keys = one 64-key block for each of the four waves, and the
// interface promises that fewer than 512 keys are never split.  The starting values (512, 256) were 5 % slower over the sweep's shapes.
#ifndef FA_KV_TARGET_WGS
#define FA_KV_TARGET_WGS 256
#endif
#ifndef FA_KV_MIN_SHARE
#define FA_KV_MIN_SHARE 256
#endif
constexpr int kKvTargetWorkgroups = FA_KV_TARGET_WGS;   // split until a launch has about this many workgroups ...
constexpr int kKvMinShareKeys = FA_KV_MIN_SHARE;        // ... but give no share fewer keys than this

struct KvPlan {
    int32_t row_tiles;   // T = ceil(group * nq / kKvRowTile)
    int32_t splits;      // S
    int32_t share;       // keys per share, a multiple of 64
};

// bh_kv, group, nq, nk as validated by the caller (all >= 1).  Inline: the paged and the fp8 library plan with the same code (fa_kv_host.h)
// and link no host object of this library.
// The M = group * nq rows of a K/V slab are packed into T tiles of kKvRowTile rows; a launch has bh_kv * T * S workgroups.
//   S = clamp(ceil(target / (bh_kv * T)), 1, min(64, nk / min_share)), share = ceil(nk / S) rounded up to 64 keys,
//   S is lowered (and the share recomputed) until the last share is not empty.
inline KvPlan kv_plan(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk)
{
    KvPlan pl;
    const int64_t m = (int64_t)group * nq;
    const int64_t tiles = (m + kKvRowTile - 1) / kKvRowTile;
    pl.row_tiles = (int32_t)tiles;
    const int64_t wgs = bh_kv * tiles;
    int64_t s = (kKvTargetWorkgroups + wgs - 1) / wgs;
    int64_t cap = nk / kKvMinShareKeys;
    if (cap > kKvMaxSplits) cap = kKvMaxSplits;
    if (s > cap) s = cap;
    if (s < 1) s = 1;
    int64_t share;
    for (;;) {   // the largest S <= s whose last share is not empty, with the share size that belongs to it
        share = ((nk + s - 1) / s + 63) / 64 * 64;
        if (s > 1 && (s - 1) * share >= nk) --s; else break;
    }
    pl.splits = (int32_t)s;
    pl.share = (int32_t)share;
    return pl;
}

inline size_t kv_workspace_bytes(const KvPlan& pl, int64_t bh_kv, int32_t group, int64_t nq, int32_t d)
{
    if (pl.splits <= 1) return 0;
    const size_t rows = (size_t)bh_kv * (size_t)group * (size_t)nq;
    return ((size_t)pl.splits * rows * (size_t)(d + 1) * 4 + 255) / 256 * 256;
}

struct KvParams {
    const void* q;          // (bh_kv * group, nq, d) bf16: the M = group * nq rows of one K/V slab are contiguous ("packed rows")
    const void* k;          // (bh_kv, capacity, d) bf16
    const void* v;
    void* o;                // (bh_kv * group, nq, d) bf16 or fp32
    float* lse;             // nullable
    const int32_t* kv_lens; // nullable, device
    float* o_part;          // S > 1: [S][bh_kv * M][d] fp32, normalised
    float* lse_part;        // S > 1: [S][bh_kv * M] fp32, natural log
    int64_t kv_slab_stride; // capacity * d, elements
    int32_t m_rows;         // M
    int32_t nq, nk;
    int32_t bh_kv;
    int32_t row_tiles, splits, share;
    float scale_log2e;
};

hipError_t launch_kv_decode(const KvParams& p, int d, int causal, int out_f32, hipStream_t stream);
hipError_t launch_kv_combine(const KvParams& p, int d, int out_f32, hipStream_t stream);
hipError_t launch_kv_stream_read(const void* k, const void* v, int64_t bh_kv, int64_t nk, int64_t capacity, int d, const KvPlan& pl,
                                 uint32_t* sink, hipStream_t stream);
const char* kv_decode_kernel_name();

}  // namespace fa
