/*
 * include/flashattn_amd_kvw.h -- C ABI of sliding-window KV-cache attention (libflashattn_amd_kvw.so), beside
 *                                include/flashattn_amd_kv.h (the contiguous cache) and include/flashattn_amd_paged.h (the paged
 *                                one), whose semantics it keeps, and the frozen include/flashattn_amd.h (ABI 6), whose status
 *                                codes and dtypes it shares.
 *
 * Models with local attention layers attend to the last W keys only.  fa_kvw_forward and fa_kvw_paged_forward are fa_kv_forward
 * and fa_paged_forward with one more argument, `window_left`, which bounds the keys a query row sees from below.  The window is
 * no mask over a full-length call: a workgroup walks only the keys its rows can see, and the host lays the key shares over that
 * range, so a windowed call over a long cache costs what fa_kv_forward costs on a cache of W keys, whatever the length is.
 *
 * Conventions are the main header's: plain C, raw device pointers, an opaque HIP stream, fa_status return codes, a thread-local
 * error text (fa_kvw_last_error), no allocation, no synchronisation, legal while `stream` is capturing; nothing on the device is
 * touched before validation passes.
 *
 * Semantics
 *   window    window_left >= 0 reads as flash-attn's window_size = (left, -1 | 0).  With len the length of a slab (of a sequence)
 *             and diag = len - nq, query row i sees key j iff
 *                    j <  len
 *                    j >= diag + i - window_left
 *                    j <= diag + i                   (causal only)
 *             causal with window_left = W - 1: "the last W keys including my own"; non-causal: the lower bound only.  The window
 *             slides per slab with its own length when kv_lens / seq_lens is given.
 *   ranges    window_left < 0: FA_ERR_INVALID_ARGUMENT.  window_left > 2^24 is treated as 2^24 (no cache is longer: nothing is
 *             hidden).  With window_left >= nk - 1 the results are those of fa_kv_forward / fa_paged_forward, bit for bit.
 *   what is read   with lo_slab = max(0, len - nq - window_left):
 *                    no K/V row < lo_slab and none >= len is read;
 *                    paged: no block-table entry < lo_slab >> log2(page_size) and none >= ceil(len / page_size) is read.
 *             Rows and table entries outside may hold anything, and their pages may be freed or reused.  Loads that a wave's
 *             64-key block would make outside the range are redirected: past the end to the last row read, below the window to
 *             the first.  The redirect acts on the logical row, before the table lookup, so a redirected row finds its page under
 *             the entry it would have used.
 *   everything else -- packed rows, GQA, kv_lens / seq_lens read on the device only, rows without a visible key (O = 0,
 *             LSE = -inf, never NaN), dtypes (FA_DTYPE_BF16, FA_DTYPE_BF16_OUT_F32; FA_DTYPE_F32: FA_ERR_UNSUPPORTED), d (64 or
 *             128), arithmetic (one bf16 product for Q.K^T, P as bf16 hi + bf16 lo, the row sum on the matrix pipe: a constant V
 *             comes out exactly), accuracy, capacity, ranges, alignment, overlap, the fa_paged_cache struct and its rules -- is word
 *             for word include/flashattn_amd_kv.h and include/flashattn_amd_paged.h.
 *   workspace as in fa_kv_forward.  The plan is laid over the widest key range a row tile can have,
 *                    span = min(nk, window_left + nq + 63)
 *             (the window, the rows of a tile, and the keys down to the 64-key boundary the tile's blocks start at), not over nk:
 *             fa_kvw_splits_for and fa_kvw_workspace_bytes return what fa_kv_splits_for and fa_kv_workspace_bytes return for a
 *             cache of `span` keys.  They depend on the shapes and on window_left only, never on lengths.  NULL or 0 bytes: the
 *             call runs unsplit.  Non-NULL but too small: FA_ERR_INVALID_ARGUMENT.  Contents need no initialisation.
 *
 * Out of scope: attention sinks, a right window other than causal / unbounded, soft-capping.  fp8 caches under a window:
 * include/flashattn_amd_kvw8.h (libflashattn_amd_kvw8.so; their decode loop is a different one).
 */
#ifndef FLASHATTN_AMD_KVW_H
#define FLASHATTN_AMD_KVW_H

#include "flashattn_amd.h"
#include "flashattn_amd_paged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLASHATTN_AMD_KVW_ABI_VERSION 1

/* Bytes of scratch fa_kvw_forward can use for these shapes and this window (0: the plan does not split). */
size_t fa_kvw_workspace_bytes(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                              int32_t window_left);

/* Number of key shares S (1 .. 64) a call with a sufficient workspace runs with; 0 for rejected arguments. */
int32_t fa_kvw_splits_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                          int32_t window_left);

/* Name of the kernel family fa_kvw_forward launches for this call, or NULL for arguments it would reject. */
const char* fa_kvw_kernel_name_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                                   int32_t window_left);

/* fa_kv_forward with a window.  Enqueues one kernel (unsplit) or two (key shares + combine) on `stream` and returns. */
int fa_kvw_forward(const void* q, const void* k, const void* v, void* o, float* lse,
                   int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int64_t capacity, const int32_t* kv_lens,
                   int32_t d, float scale, int32_t causal, int32_t dtype, int32_t window_left,
                   void* workspace, size_t workspace_bytes, void* stream);

/* The same three for a paged cache: what the contiguous ones return at bh_kv = batch * heads_kv. */
size_t fa_kvw_paged_workspace_bytes(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal,
                                    int32_t dtype, int32_t window_left);
int32_t fa_kvw_paged_splits_for(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal,
                                int32_t dtype, int32_t window_left);

/* fa_paged_forward with a window. */
int fa_kvw_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse,
                         int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d,
                         float scale, int32_t causal, int32_t dtype, int32_t window_left,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Thread-local description of the last failure of an fa_kvw_* call on this thread ("" if none). */
const char* fa_kvw_last_error(void);

/* "flashattn_amd_kvw abi <n> gfx950 ..." build string. */
const char* fa_kvw_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FLASHATTN_AMD_KVW_H */
