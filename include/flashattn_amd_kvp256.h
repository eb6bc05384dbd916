/*
 * include/flashattn_amd_kvp256.h -- C ABI of chunked prefill over the bf16 K/V caches at head dim 256 (libflashattn_amd_kvp256.so),
 *                                   beside include/flashattn_amd_kvp.h (the same two calls at head dim 128) and
 *                                   include/flashattn_amd_kv256.h (the decode kernels at head dim 256), whose semantics it keeps
 *                                   for calls with MANY query rows, and the frozen include/flashattn_amd.h (ABI 6), whose status
 *                                   codes and dtypes it shares.
 *
 * fa_kv256_forward and fa_kv256_paged_forward run a decode kernel: a workgroup owns 32 packed query rows and streams the whole K/V
 * slab for them, which re-reads the slab once per 32 rows for a 2048-token chunk.  fa_kvp256_forward and fa_kvp256_paged_forward
 * are the same two calls on a kernel built for the other regime: a workgroup owns 128 packed rows, its four waves walk the same
 * 64-key blocks, and every block passes through LDS once per workgroup (docs/kv_prefill_d256.md has the design and the
 * measurements).  There is no key split: the calls take no workspace.
 *
 * Conventions are the main header's: plain C, raw device pointers, an opaque HIP stream, fa_status return codes, a thread-local
 * error text (fa_kvp256_last_error), no allocation, no synchronisation, legal while `stream` is capturing; nothing on the device
 * is touched before validation passes.  kv_lens / seq_lens and the block table are read on the device only.
 *
 * Semantics
 *   d         256.  Anything else: FA_ERR_UNSUPPORTED ("head dim 128 is not supported: 256").
 *   dtypes    FA_DTYPE_BF16 and FA_DTYPE_BF16_OUT_F32; FA_DTYPE_F32: FA_ERR_UNSUPPORTED.
 *   what is read   no K/V row at or beyond len (the slab's kv_lens / the sequence's seq_lens entry, clamped to [0, nk]); paged:
 *             no block-table entry at or beyond ceil(len / page_size).  Loads that a 64-key block would make past the last
 *             visible row are redirected to it, on the logical row and before the table lookup.
 *   everything else -- packed rows (bh_kv * group, nq, d), GQA, bottom-right aligned causal masking (j <= len - nq + i), rows
 *             without a visible key (O = 0, LSE = -inf, never NaN), arithmetic (one bf16 product for Q.K^T, P as bf16 hi +
 *             bf16 lo, the row sum on the matrix pipe: a constant V comes out exactly), ranges, alignment, overlap, the 2^32-byte
 *             slab limit, the fa_paged_cache struct and its rules (pages of 16 .. 65536 rows, a power of two) -- is word for word
 *             include/flashattn_amd_kvp.h.  The results agree with include/flashattn_amd_kv256.h's to their common accuracy, not
 *             bit for bit (other block boundaries per row); fa_kvp256_paged_forward equals fa_kvp256_forward on the gathered
 *             cache bit for bit.
 *
 * window_left is served by include/flashattn_amd_kvpw.h (libflashattn_amd_kvpw.so).
 * Out of scope: fp8 caches at this head dim, a key split for grids of a few workgroups (bh_kv * ceil(group * nq / 128)
 * well below the 256 CUs), and routing from fa_kv256_forward / fa_kv256_paged_forward, which keep their kernels and their bits.
 */
#ifndef FLASHATTN_AMD_KVP256_H
#define FLASHATTN_AMD_KVP256_H

#include "flashattn_amd.h"
#include "flashattn_amd_paged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLASHATTN_AMD_KVP256_ABI_VERSION 1

/* Name of the kernel family fa_kvp256_forward launches for this call, or NULL for arguments it would reject. */
const char* fa_kvp256_kernel_name_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype);

/* Enqueues one kernel on `stream` and returns.  The arguments are fa_kvp_forward's. */
int fa_kvp256_forward(const void* q, const void* k, const void* v, void* o, float* lse,
                      int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int64_t capacity, const int32_t* kv_lens,
                      int32_t d, float scale, int32_t causal, int32_t dtype, void* stream);

/* The same for a paged cache: fa_kvp_paged_forward's arguments. */
int fa_kvp256_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse,
                            int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d,
                            float scale, int32_t causal, int32_t dtype, void* stream);

/* Thread-local description of the last failure of an fa_kvp256_* call on this thread ("" if none). */
const char* fa_kvp256_last_error(void);

/* "flashattn_amd_kvp256 abi <n> gfx950 ..." build string. */
const char* fa_kvp256_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FLASHATTN_AMD_KVP256_H */
