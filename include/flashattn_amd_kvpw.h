/*
 * include/flashattn_amd_kvpw.h -- C ABI of chunked prefill under a sliding window (libflashattn_amd_kvpw.so), beside
 *                                 include/flashattn_amd_kvp.h, include/flashattn_amd_kvp256.h and include/flashattn_amd_kvp8.h
 *                                 (the same calls without a window), whose kernels, caches and rules it keeps, and
 *                                 include/flashattn_amd_kvw.h (the decode kernels under a window), whose window it keeps.
 *                                 Status codes and dtypes are those of the frozen include/flashattn_amd.h (ABI 6).
 *
 * A model with a sliding window could carry a chunk of nq rows through its cache only on the decode kernels (fa_kvw_forward and
 * its twins): 32-row workgroups that re-read the window once per 32 packed rows.  These calls run the chunked-prefill kernels --
 * 256 packed rows per workgroup at d = 128, 128 at d = 256, every 64-key block through LDS once per workgroup -- over the keys of
 * the window alone: a tile walks the 64-key blocks from the one that holds its lowest row's first key to the one that holds its
 * widest row's last, so the time of a call follows window_left + nq, not the length of the cache (docs/kv_prefill_window.md has
 * the design and the measurements).  There is no key split: the calls take no workspace.
 *
 * Conventions are the main header's: plain C, raw device pointers, an opaque HIP stream, fa_status return codes, a thread-local
 * error text (fa_kvpw_last_error), no allocation, no synchronisation, legal while `stream` is capturing; nothing on the device
 * is touched before validation passes.  kv_lens / seq_lens and the block table are read on the device only.
 *
 * Semantics
 *   window    exactly include/flashattn_amd_kvw.h: with len the slab's length, query row i sees key j iff j < len,
 *             j >= len - nq + i - window_left and, when causal, j <= len - nq + i.  window_left is 0 .. 2^24; below 0:
 *             FA_ERR_INVALID_ARGUMENT ("window_left = -1 must be >= 0"); wider than 2^24 is taken as 2^24 and hides nothing.
 *             With window_left >= nk the result is, bit for bit, that of the unwindowed call of the same cache.
 *   what is read   with lo = max(0, len - nq - window_left): no K/V row below lo and none at or beyond len; paged: no block-table
 *             entry of a page wholly below lo and none at or beyond ceil(len / page_size).  Such rows, pages and entries may hold
 *             anything (fp8: the NaN codes included).  Loads that a 64-key block would make outside the tile's keys are
 *             redirected to the nearest row inside, on the logical row and before the table lookup.
 *   d, dtypes fa_kvpw_forward / fa_kvpw_paged_forward: bf16 caches at d = 128 or 256 ("head dim 64 is not supported: 128 or 256");
 *             fa_kvpw_fp8_forward / fa_kvpw_fp8_paged_forward: e4m3fn caches at d = 128 ("head dim 256 is not supported: 128"),
 *             with the cache, k_scale and v_scale of include/flashattn_amd_kvp8.h.  FA_DTYPE_BF16 and FA_DTYPE_BF16_OUT_F32 for
 *             q and o; FA_DTYPE_F32: FA_ERR_UNSUPPORTED.
 *   contract  everything else is the unwindowed header's of the same cache and head dim: packed rows, GQA, rows without a visible
 *             key (O = 0, LSE = -inf, never NaN), the arithmetic, ranges, alignment, overlap, the fa_paged_cache struct.  A paged
 *             call equals the contiguous one on the gathered cache bit for bit; with v_scale a power of two an fp8 call gives,
 *             bit for bit, v_scale x what fa_kvpw_forward gives on the cache dequantised to bf16 at fp32(scale * k_scale), and
 *             its LSE for any v_scale.  The results agree with fa_kvw_forward's to their common accuracy, not bit for bit.
 *
 * Out of scope: fp8 caches at head dim 256, head dim 64, a key split for grids of a few workgroups, a right-hand window other
 * than causal / none, and routing between these calls and the decode kernels.
 */
#ifndef FLASHATTN_AMD_KVPW_H
#define FLASHATTN_AMD_KVPW_H

#include "flashattn_amd.h"
#include "flashattn_amd_paged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLASHATTN_AMD_KVPW_ABI_VERSION 1

/* Name of the kernel family fa_kvpw_forward launches for this call, or NULL for arguments it would reject. */
const char* fa_kvpw_kernel_name_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                                    int32_t window_left);

/* Enqueues one kernel on `stream` and returns.  The arguments are fa_kvp_forward's with window_left behind dtype. */
int fa_kvpw_forward(const void* q, const void* k, const void* v, void* o, float* lse,
                    int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int64_t capacity, const int32_t* kv_lens,
                    int32_t d, float scale, int32_t causal, int32_t dtype, int32_t window_left, void* stream);

/* The same for a paged cache: fa_kvp_paged_forward's arguments with window_left behind dtype. */
int fa_kvpw_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse,
                          int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d,
                          float scale, int32_t causal, int32_t dtype, int32_t window_left, void* stream);

/* The same two over an fp8 (e4m3fn) cache: fa_kvp8_forward's and fa_kvp8_paged_forward's arguments with window_left behind dtype. */
int fa_kvpw_fp8_forward(const void* q, const void* k8, const void* v8, void* o, float* lse,
                        int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int64_t capacity, const int32_t* kv_lens,
                        int32_t d, float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype, int32_t window_left, void* stream);

int fa_kvpw_fp8_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse,
                              int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d,
                              float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype, int32_t window_left, void* stream);

/* Thread-local description of the last failure of an fa_kvpw_* call on this thread ("" if none). */
const char* fa_kvpw_last_error(void);

/* "flashattn_amd_kvpw abi <n> gfx950 ..." build string. */
const char* fa_kvpw_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FLASHATTN_AMD_KVPW_H */
