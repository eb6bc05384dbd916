/*
 * include/flashattn_amd_kv256.h -- C ABI of KV-cache attention at head dim 256 (libflashattn_amd_kv256.so), beside
 *                                  include/flashattn_amd_kv.h (the contiguous cache), include/flashattn_amd_paged.h (the paged
 *                                  one) and include/flashattn_amd_kvw.h (the sliding window), whose semantics it keeps at the
 *                                  one head dim their kernels do not reach, and the frozen include/flashattn_amd.h (ABI 6),
 *                                  whose status codes and dtypes it shares.
 *
 * Models with 256-wide heads (GQA, a sliding window on every other layer) prefill through fa_forward, which takes any head dim
 * up to 256; this library decodes for them.  fa_kv256_forward and fa_kv256_paged_forward are fa_kvw_forward and
 * fa_kvw_paged_forward with d = 256 and with window_left = -1 standing for "no window" (then they are fa_kv_forward and
 * fa_paged_forward).  The decode kernel is its own: it walks the keys in blocks of 32 instead of 64, which is what the LDS, the
 * load counter and the register file of a CU allow at this width (docs/kv_d256.md).
 *
 * Conventions are the main header's: plain C, raw device pointers, an opaque HIP stream, fa_status return codes, a thread-local
 * error text (fa_kv256_last_error), no allocation, no synchronisation, legal while `stream` is capturing; nothing on the device
 * is touched before validation passes.  kv_lens / seq_lens and the block table are read on the device only.
 *
 * Semantics
 *   d         256.  Anything else: FA_ERR_UNSUPPORTED ("head dim 128 is not supported: 256"); 64 and 128 are served by the
 *             libraries named above.
 *   dtypes    FA_DTYPE_BF16 and FA_DTYPE_BF16_OUT_F32; FA_DTYPE_F32: FA_ERR_UNSUPPORTED.
 *   window    window_left = -1: no window.  window_left >= 0: as in include/flashattn_amd_kvw.h -- with len the length of a
 *             slab (of a sequence) and diag = len - nq, query row i sees key j iff j < len, j >= diag + i - window_left and,
 *             causal only, j <= diag + i.  window_left < -1: FA_ERR_INVALID_ARGUMENT.  window_left > 2^24 is treated as 2^24;
 *             with window_left >= nk - 1 the results are those of window_left = -1, bit for bit.
 *   what is read   with lo_slab = max(0, len - nq - window_left) (0 without a window): no K/V row < lo_slab and none >= len is
 *             read; paged: no block-table entry < lo_slab >> log2(page_size) and none >= ceil(len / page_size).  Loads that a
 *             wave's 32-key block would make outside the range are redirected, on the logical row and before the table lookup:
 *             past the end to the last row read, below the window to the first.
 *   capacity  a K/V slab must stay below 2^32 bytes: capacity * d * 2 < 2^32, which at d = 256 is capacity < 2^23 rows
 *             (FA_ERR_UNSUPPORTED at 2^23 and above).  nk <= 2^24 as everywhere, so the capacity is the limit that binds.
 *   everything else -- packed rows, GQA, bottom-right aligned causal masking, rows without a visible key (O = 0, LSE = -inf,
 *             never NaN), arithmetic (one bf16 product for Q.K^T, P as bf16 hi + bf16 lo, the row sum on the matrix pipe: a
 *             constant V comes out exactly), ranges, alignment, overlap, the fa_paged_cache struct and its rules (pages of
 *             16 .. 65536 rows, a power of two) -- is word for word include/flashattn_amd_kv.h and include/flashattn_amd_paged.h.
 *   workspace as in fa_kv_forward.  Without a window the plan is laid over nk; with one over
 *                    span = min(nk, window_left + nq + 63)
 *             exactly as in include/flashattn_amd_kvw.h (key shares start at multiples of 64 keys here too).  The queries depend
 *             on the shapes and on window_left only, never on lengths.  NULL or 0 bytes: the call runs unsplit.  Non-NULL but
 *             too small: FA_ERR_INVALID_ARGUMENT.  Contents need no initialisation.
 *
 * fp8 caches at d = 256: include/flashattn_amd_kv8_256.h.  Out of scope: head dims 96, 160 and 192.
 */
#ifndef FLASHATTN_AMD_KV256_H
#define FLASHATTN_AMD_KV256_H

#include "flashattn_amd.h"
#include "flashattn_amd_paged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLASHATTN_AMD_KV256_ABI_VERSION 1

/* Bytes of scratch fa_kv256_forward can use for these shapes and this window (0: the plan does not split). */
size_t fa_kv256_workspace_bytes(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                                int32_t window_left);

/* Number of key shares S (1 .. 64) a call with a sufficient workspace runs with; 0 for rejected arguments. */
int32_t fa_kv256_splits_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                            int32_t window_left);

/* Name of the kernel family fa_kv256_forward launches for this call, or NULL for arguments it would reject. */
const char* fa_kv256_kernel_name_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                                     int32_t window_left);

/* Enqueues one kernel (unsplit) or two (key shares + combine) on `stream` and returns. */
int fa_kv256_forward(const void* q, const void* k, const void* v, void* o, float* lse,
                     int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int64_t capacity, const int32_t* kv_lens,
                     int32_t d, float scale, int32_t causal, int32_t dtype, int32_t window_left,
                     void* workspace, size_t workspace_bytes, void* stream);

/* The same for a paged cache: the queries return what the contiguous ones return at bh_kv = batch * heads_kv. */
size_t fa_kv256_paged_workspace_bytes(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal,
                                      int32_t dtype, int32_t window_left);
int32_t fa_kv256_paged_splits_for(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal,
                                  int32_t dtype, int32_t window_left);

int fa_kv256_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse,
                           int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d,
                           float scale, int32_t causal, int32_t dtype, int32_t window_left,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Thread-local description of the last failure of an fa_kv256_* call on this thread ("" if none). */
const char* fa_kv256_last_error(void);

/* "flashattn_amd_kv256 abi <n> gfx950 ..." build string. */
const char* fa_kv256_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FLASHATTN_AMD_KV256_H */
