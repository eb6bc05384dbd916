/*
 * include/flashattn_amd_kvw8.h -- C ABI of sliding-window KV-cache attention over a cache of 8-bit floats
 *                                 (libflashattn_amd_kvw8.so): include/flashattn_amd_kv8.h (the fp8 e4m3fn cache, contiguous and
 *                                 paged) under the window of include/flashattn_amd_kvw.h.  It keeps the semantics of both and shares
 *                                 the status codes and dtypes of the frozen include/flashattn_amd.h (ABI 6).
 *
 * A model with local-attention layers served from an fp8 cache wants both halves: one byte per K/V element, and a workgroup that
 * walks only the keys its rows can see.  fa_kvw8_forward and fa_kvw8_paged_forward are fa_kv8_forward and fa_kv8_paged_forward with
 * one more argument, `window_left`, after `dtype` -- where fa_kvw_forward has it.
 *
 * Conventions are the main header's: plain C, raw device pointers, an opaque HIP stream, fa_status return codes, a thread-local
 * error text (fa_kvw8_last_error), no allocation, no synchronisation, legal while `stream` is capturing; nothing on the device is
 * touched before validation passes.
 *
 * Semantics
 *   window    word for word include/flashattn_amd_kvw.h.  With len the length of a slab (of a sequence) and diag = len - nq, query
 *             row i sees key j iff
 *                    j <  len
 *                    j >= diag + i - window_left
 *                    j <= diag + i                   (causal only)
 *             window_left < 0: FA_ERR_INVALID_ARGUMENT ("window_left = %d must be >= 0").  window_left > 2^24 is treated as 2^24 (no
 *             cache is longer: nothing is hidden).
 *   what is read   with lo_slab = max(0, len - nq - window_left):
 *                    no cache byte of a row < lo_slab and none of a row >= len is read;
 *                    paged: no block-table entry < lo_slab >> log2(page_size) and none >= ceil(len / page_size) is read.
 *             Loads that a wave's 64-key block would make outside the range are redirected on the logical row, before the table
 *             lookup: past the end to the last row read, below the window to the tile's first visible row.  Rows and table entries
 *             outside may hold anything, the NaN codes 0x7F / 0xFF included, and their pages may be freed or reused.  This matters
 *             more here than in the 16-bit library: a redirected row carries weight zero in P.V, and a NaN code that met that zero
 *             would come out as NaN -- it is never loaded.
 *   cache, scales, arithmetic   word for word include/flashattn_amd_kv8.h: one byte per element (OCP e4m3fn), strides and capacities in
 *             elements, caches and pools 16-byte aligned, paged strides multiples of 16 elements; k_scale and v_scale finite and
 *             > 0; k_scale is folded into `scale` as ONE fp32 product; v_scale multiplies the normalised fp32 result once, in front
 *             of the store to o (unsplit) or behind the merge of the shares (split).  The LSE does not contain v_scale.
 *   plan      that of include/flashattn_amd_kvw.h, laid over span = min(nk, window_left + nq + 63): fa_kvw8_splits_for and
 *             fa_kvw8_workspace_bytes return what fa_kvw_splits_for and fa_kvw_workspace_bytes return for the same arguments (the
 *             paged queries: what the contiguous ones return at bh_kv = batch * heads_kv).  They depend on the shapes and on
 *             window_left only, never on lengths.  Workspace NULL or 0 bytes: the call runs unsplit.  Non-NULL but too small:
 *             FA_ERR_INVALID_ARGUMENT.
 *   bits      1. with v_scale a power of two, O is v_scale x what fa_kvw_forward / fa_kvw_paged_forward give on the cache dequantised
 *                to bf16 with scale' = fp32(scale * k_scale) and the same window_left, bit for bit; the LSE is bit-identical for any
 *                v_scale;
 *             2. with window_left >= nk - 1 the results are those of fa_kv8_forward / fa_kv8_paged_forward, bit for bit;
 *             3. the paged entry equals the contiguous one on the gathered bytes, bit for bit.
 *
 * Out of scope: attention sinks, soft-capping, a right window other than causal / unbounded, per-head or per-token scales (and
 * what include/flashattn_amd_kv8.h leaves out: e5m2 and the fnuz encodings, an fp8 q, a kernel that quantises or appends rows).
 */
#ifndef FLASHATTN_AMD_KVW8_H
#define FLASHATTN_AMD_KVW8_H

#include "flashattn_amd.h"
#include "flashattn_amd_paged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLASHATTN_AMD_KVW8_ABI_VERSION 1

/* Bytes of scratch fa_kvw8_forward can use for these shapes and this window (0: the plan does not split). */
size_t fa_kvw8_workspace_bytes(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                               int32_t window_left);

/* Number of key shares S (1 .. 64) a call with a sufficient workspace runs with; 0 for rejected arguments. */
int32_t fa_kvw8_splits_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                           int32_t window_left);

/* Name of the kernel family a forward launches for this call (page_size 0: the contiguous cache), or NULL for arguments it would reject. */
const char* fa_kvw8_kernel_name_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                                    int32_t page_size, int32_t window_left);

/* fa_kv8_forward with a window.  Enqueues one kernel (unsplit) or two (key shares + combine) on `stream` and returns. */
int fa_kvw8_forward(const void* q, const void* k8, const void* v8, void* o, float* lse,
                    int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int64_t capacity, const int32_t* kv_lens,
                    int32_t d, float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype, int32_t window_left,
                    void* workspace, size_t workspace_bytes, void* stream);

/* The two queries for a paged cache: what the contiguous ones return at bh_kv = batch * heads_kv. */
size_t fa_kvw8_paged_workspace_bytes(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal,
                                     int32_t dtype, int32_t window_left);
int32_t fa_kvw8_paged_splits_for(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal,
                                 int32_t dtype, int32_t window_left);

/* fa_kv8_paged_forward with a window: the struct of flashattn_amd_paged.h, its pools read as e4m3 bytes. */
int fa_kvw8_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse,
                          int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d,
                          float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype, int32_t window_left,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Thread-local description of the last failure of an fa_kvw8_* call on this thread ("" if none). */
const char* fa_kvw8_last_error(void);

/* "flashattn_amd_kvw8 abi <n> gfx950 ..." build string. */
const char* fa_kvw8_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FLASHATTN_AMD_KVW8_H */
