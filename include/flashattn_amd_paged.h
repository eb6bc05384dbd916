/*
 * include/flashattn_amd_paged.h -- C ABI of paged KV-cache attention (libflashattn_amd_paged.so), beside include/flashattn_amd_kv.h
 *                                  (the contiguous cache), whose semantics it keeps, and the frozen include/flashattn_amd.h (ABI 6),
 *                                  whose status codes and dtypes it shares.
 *
 * The cache of a serving engine: K and V rows live in fixed-size pages of one shared pool, and a per-sequence block table maps
 * logical pages to physical ones, so sequences grow, are evicted and share prefixes without a copy.  fa_paged_forward reads the
 * pages where they are -- no gather pass in front of the forward.
 *
 * Conventions are the main header's: plain C, raw device pointers, an opaque HIP stream, fa_status return codes, a thread-local
 * error text (fa_paged_last_error), no allocation, no synchronisation, legal while `stream` is capturing; nothing on the device is
 * touched before validation passes.
 *
 * Semantics
 *   tensors   q, o : (batch * heads_kv * group, nq, d) row-major contiguous; query slab ((b * heads_kv) + h) * group + g reads K/V
 *                    head h of sequence b
 *             lse  : NULL or (batch * heads_kv * group, nq) fp32, natural log
 *   cache     key row j of head h of sequence b is the d elements at
 *                    k_pool + block_table[b][j / page_size] * page_stride + (j % page_size) * row_stride + h * head_stride
 *             (elements; the page base is formed in 64 bits), the value row likewise in v_pool.  One block table and one length per
 *             sequence, shared by its heads.  The strides cover
 *                    (pages, page, d), heads_kv = 1       page_stride = page * d       row_stride = d       head_stride = 0
 *                    (pages, page, H, d)                  page_stride = page * H * d   row_stride = H * d   head_stride = d
 *                    (pages, H, page, d)                  page_stride = H * page * d   row_stride = d       head_stride = page * d
 *   lengths   seq_lens: NULL (every sequence has nk keys) or a DEVICE pointer to int32[batch], each value clamped to [0, nk]
 *   what is read   with len the length of a sequence: pool rows are read only where they hold one of its first len keys.  The tail
 *             of its last page is never read; a page that no table entry below ceil(len / page_size) names is never read; table
 *             entries at or beyond ceil(len / page_size) are never read and may hold anything.  Entries below that must lie in
 *             [0, num_pages).  The host never dereferences the table or the lengths: one captured graph follows a cache that
 *             grows and whose pages move.  Two sequences may name the same physical page (prefix sharing): pages are read-only.
 *   math, causal (bottom-right aligned), rows without keys (O = 0, LSE = -inf, never NaN), dtypes (FA_DTYPE_BF16,
 *             FA_DTYPE_BF16_OUT_F32; FA_DTYPE_F32: FA_ERR_UNSUPPORTED), d (64 or 128), arithmetic (P as bf16 hi + bf16 lo, the row
 *             sum on the matrix pipe: a constant V comes out exactly) and accuracy: word for word include/flashattn_amd_kv.h.  The
 *             result is that of fa_kv_forward on the gathered cache.
 *   pages     page_size a power of two, 16 .. 65536 rows (anything else: FA_ERR_UNSUPPORTED); num_pages, max_pages >= 1;
 *             nk <= max_pages * page_size, otherwise FA_ERR_INVALID_ARGUMENT; page_stride, row_stride, head_stride multiples of 8
 *             elements (16 bytes), row_stride >= d, page_stride >= 1, head_stride >= 0.  A pool may exceed 2^32 bytes; the offset
 *             inside a page, page_size * row_stride * 2 bytes plus the head offset (heads_kv - 1) * head_stride * 2, must stay
 *             below 2^32 bytes: larger gives FA_ERR_UNSUPPORTED
 *   ranges    batch, heads_kv, group, nq, nk >= 1; nk <= 2^24; group * nq <= 2^30; batch * heads_kv * group <= 2^31 - 1
 *   alignment q, o, k_pool, v_pool 16 bytes; lse, block_table, seq_lens 4; workspace 256
 *   overlap   o, lse and the workspace must overlap neither pool -- measured over its whole strided extent, (num_pages - 1) *
 *             page_stride plus one page -- nor the table, the lengths or q: FA_ERR_INVALID_ARGUMENT
 *   workspace as in fa_kv_forward.  The plan is that of the contiguous cache with bh_kv = batch * heads_kv: fa_paged_splits_for and
 *             fa_paged_workspace_bytes return what fa_kv_splits_for and fa_kv_workspace_bytes return for those shapes.  NULL or 0
 *             bytes: the call runs unsplit.  Non-NULL but too small: FA_ERR_INVALID_ARGUMENT.  Contents need no initialisation.
 *
 * Out of scope: a kernel that appends rows to the cache (callers scatter new rows with their own indexing), fp8 pages, and page
 * sizes that are not powers of two.
 */
#ifndef FLASHATTN_AMD_PAGED_H
#define FLASHATTN_AMD_PAGED_H

#include "flashattn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLASHATTN_AMD_PAGED_ABI_VERSION 1

typedef struct fa_paged_cache {
    const void* k_pool;          /* bf16 */
    const void* v_pool;
    int64_t num_pages;
    int32_t page_size;           /* rows per page: a power of two, 16 .. 65536 */
    int64_t page_stride;         /* elements; each stride a multiple of 8 (16 bytes) */
    int64_t row_stride;          /* >= d */
    int64_t head_stride;
    const int32_t* block_table;  /* DEVICE, int32 [batch][max_pages]; entry p of sequence b = physical page of rows [p * page_size, (p + 1) * page_size) */
    int32_t max_pages;
    const int32_t* seq_lens;     /* NULL (every sequence has nk keys) or DEVICE int32[batch], clamped to [0, nk] */
} fa_paged_cache;

/* Bytes of scratch fa_paged_forward can use for these shapes (0: the plan does not split). */
size_t fa_paged_workspace_bytes(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype);

/* Number of key shares S (1 .. 64) a call with a sufficient workspace runs with; 0 for rejected arguments. */
int32_t fa_paged_splits_for(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype);

/* Name of the kernel family fa_paged_forward launches for this call, or NULL for arguments it would reject. */
const char* fa_paged_kernel_name_for(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                                     int32_t page_size);

/* The forward.  Enqueues one kernel (unsplit) or two (key shares + combine) on `stream` and returns. */
int fa_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse,
                     int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d,
                     float scale, int32_t causal, int32_t dtype, void* workspace, size_t workspace_bytes, void* stream);

/* Thread-local description of the last failure of an fa_paged_* call on this thread ("" if none). */
const char* fa_paged_last_error(void);

/* "flashattn_amd_paged abi <n> gfx950 ..." build string. */
const char* fa_paged_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FLASHATTN_AMD_PAGED_H */
