/*
 * include/flashattn_amd_kv8_256.h -- C ABI of KV-cache attention at head dim 256 over a cache of 8-bit floats
 *                                    (libflashattn_amd_kv8_256.so), beside include/flashattn_amd_kv256.h (the same head dim over
 *                                    a bf16 cache), whose nine symbols it carries under the prefix fa_kv8_256_, and
 *                                    include/flashattn_amd_kv8.h / include/flashattn_amd_kvw8.h (fp8 caches at d = 64 and 128),
 *                                    whose element type, scales and arithmetic contract it keeps.
 *
 * fa_kv8_256_forward and fa_kv8_256_paged_forward are fa_kvw8_forward and fa_kvw8_paged_forward with d = 256 and with
 * window_left = -1 standing for "no window" (then they are fa_kv8_forward and fa_kv8_paged_forward).  The decode kernel is its
 * own: the 32-key block of the d = 256 library with the data movement of the fp8 ones (docs/kv_fp8_d256.md).
 *
 * Conventions are the main header's: plain C, raw device pointers, an opaque HIP stream, fa_status return codes, a thread-local
 * error text (fa_kv8_256_last_error), no allocation, no synchronisation, legal while `stream` is capturing; nothing on the
 * device is touched before validation passes.  kv_lens / seq_lens and the block table are read on the device only.
 *
 * Semantics
 *   d         256.  Anything else: FA_ERR_UNSUPPORTED ("head dim 128 is not supported: 256"); 64 and 128 are served by
 *             include/flashattn_amd_kv8.h and include/flashattn_amd_kvw8.h.
 *   dtypes    q: bf16.  k8 / v8 and the pools: OCP e4m3fn, one byte per element; every stride of fa_paged_cache counts bytes.
 *             FA_DTYPE_BF16 and FA_DTYPE_BF16_OUT_F32 name the output; FA_DTYPE_F32: FA_ERR_UNSUPPORTED.
 *   scales    logical K = k_scale x the stored values, logical V = v_scale x them; both finite and > 0, scale finite and
 *             non-zero, and so is fp32(scale * k_scale) (FA_ERR_INVALID_ARGUMENT otherwise).
 *   arithmetic  the contract of include/flashattn_amd_kv8.h: e4m3 -> bf16 is exact, K and V are dequantised without their
 *             scales and meet the instruction sequence of the bf16 kernel at d = 256; k_scale is folded into scale on the host
 *             as ONE fp32 product; v_scale multiplies the normalised fp32 result once (in the decode kernel of an unsplit
 *             launch, in the merge of a split one).  Hence, with v_scale a power of two, O is bit for bit v_scale x
 *             fa_kv256_forward on the dequantised cache at scale' = fp32(scale * k_scale) with the same window_left; the LSE is
 *             bit-identical for any v_scale; the paged entry equals the contiguous one on the gathered bytes, bit for bit.
 *   window    window_left = -1: no window.  window_left >= 0: as in include/flashattn_amd_kvw.h.  window_left < -1:
 *             FA_ERR_INVALID_ARGUMENT.  window_left > 2^24 is treated as 2^24.
 *   what is read   with lo_slab = max(0, len - nq - window_left) (0 without a window): no K/V byte of a row < lo_slab or
 *             >= len is read; paged: no block-table entry < lo_slab >> log2(page_size) and none >= ceil(len / page_size).
 *             Such rows and entries may hold anything, the NaN codes 0x7F / 0xFF included.
 *   capacity  a K/V slab must stay below 2^32 bytes (a lane's offset into it has 32 bits): capacity * d < 2^32 at one byte
 *             per element, which at d = 256 is capacity < 2^24 rows (FA_ERR_UNSUPPORTED at 2^24 and above).  nk <= 2^24 as
 *             everywhere and nk <= capacity, so the bound that binds is nk <= 2^24 - 1.
 *   pools     page_stride, row_stride and head_stride are multiples of 16 bytes; pages of 16 .. 65536 rows, a power of two.
 *   workspace as in fa_kv256_forward: the plan is laid over nk without a window, over min(nk, window_left + nq + 63) with one;
 *             the partials are fp32 whatever the cache holds, so the sizes are those of include/flashattn_amd_kv256.h.
 *   everything else is word for word include/flashattn_amd_kv256.h.
 *
 * Out of scope: fp8 caches at head dims 96, 160 and 192; per-head or per-token scales.
 */
#ifndef FLASHATTN_AMD_KV8_256_H
#define FLASHATTN_AMD_KV8_256_H

#include "flashattn_amd.h"
#include "flashattn_amd_paged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLASHATTN_AMD_KV8_256_ABI_VERSION 1

/* Bytes of scratch fa_kv8_256_forward can use for these shapes and this window (0: the plan does not split). */
size_t fa_kv8_256_workspace_bytes(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                                  int32_t window_left);

/* Number of key shares S (1 .. 64) a call with a sufficient workspace runs with; 0 for rejected arguments. */
int32_t fa_kv8_256_splits_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                              int32_t window_left);

/* Name of the kernel family fa_kv8_256_forward launches for this call, or NULL for arguments it would reject. */
const char* fa_kv8_256_kernel_name_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                                       int32_t window_left);

/* Enqueues one kernel (unsplit) or two (key shares + combine) on `stream` and returns. */
int fa_kv8_256_forward(const void* q, const void* k8, const void* v8, void* o, float* lse,
                       int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int64_t capacity, const int32_t* kv_lens,
                       int32_t d, float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype, int32_t window_left,
                       void* workspace, size_t workspace_bytes, void* stream);

/* The same for a paged cache: the queries return what the contiguous ones return at bh_kv = batch * heads_kv. */
size_t fa_kv8_256_paged_workspace_bytes(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal,
                                        int32_t dtype, int32_t window_left);
int32_t fa_kv8_256_paged_splits_for(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal,
                                    int32_t dtype, int32_t window_left);

int fa_kv8_256_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse,
                             int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d,
                             float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype, int32_t window_left,
                             void* workspace, size_t workspace_bytes, void* stream);

/* Thread-local description of the last failure of an fa_kv8_256_* call on this thread ("" if none). */
const char* fa_kv8_256_last_error(void);

/* "flashattn_amd_kv8_256 abi <n> gfx950 ..." build string. */
const char* fa_kv8_256_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FLASHATTN_AMD_KV8_256_H */
