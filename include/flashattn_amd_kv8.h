/*
 * include/flashattn_amd_kv8.h -- C ABI of KV-cache attention over a cache of 8-bit floats (libflashattn_amd_kv8.so), beside
 *                                include/flashattn_amd_kv.h (the contiguous bf16 cache) and include/flashattn_amd_paged.h (the paged
 *                                one), whose semantics it keeps, and the frozen include/flashattn_amd.h (ABI 6), whose status codes
 *                                and dtypes it shares.
 *
 * The decode kernels of those two libraries run at the rate of a streaming read of their K/V bytes; only fewer bytes make them
 * faster.  Here K and V hold one byte per element, OCP e4m3fn (torch.float8_e4m3fn), with one scale per tensor and call.
 *
 * Conventions are the main header's: plain C, raw device pointers, an opaque HIP stream, fa_status return codes, a thread-local
 * error text (fa_kv8_last_error), no allocation, no synchronisation, legal while `stream` is capturing; nothing on the device is
 * touched before validation passes.
 *
 * Semantics: word for word those of fa_kv_forward (fa_kv8_forward) and fa_paged_forward (fa_kv8_paged_forward) -- packed rows, GQA,
 * bottom-right aligned causal masking, kv_lens / seq_lens read on the device only, rows without keys (O = 0, LSE = -inf), ranges,
 * the workspace and overlap rules -- except:
 *   cache     k8, v8 (or the pools of the fa_paged_cache, which is reused with its pools read as e4m3) hold one byte per element.
 *             Strides and capacities are in elements, and an element is one byte.  Caches and pools are 16-byte aligned; the paged
 *             strides are multiples of 16 elements.  A contiguous slab stays below 2^32 bytes (capacity * d); the offset inside a
 *             page, page_size * row_stride plus the head offset (heads_kv - 1) * head_stride, stays below 2^32 bytes: larger gives
 *             FA_ERR_UNSUPPORTED.  Rows at or beyond a length and the tail of a last page are never read and may hold anything,
 *             the NaN codes 0x7F / 0xFF included.  A NaN code in a row that is read behaves as a bf16 NaN would there.
 *   scales    two host floats per call: logical K = k_scale * dequant(k8), logical V = v_scale * dequant(v8).  Both finite and > 0,
 *             and scale * k_scale (fp32) finite and non-zero; otherwise FA_ERR_INVALID_ARGUMENT.
 *   arithmetic  e4m3 -> bf16 is exact for all 254 non-NaN codes: the kernel dequantises to bf16 WITHOUT the scales and runs the
 *             instruction sequence of the bf16 kernels (one bf16 product for Q.K^T into fp32, P as bf16 hi + bf16 lo, the row sum on
 *             the matrix pipe, the same contraction order over d and over keys, the same merge).  k_scale is folded into the softmax
 *             scale on the host as ONE fp32 product scale * k_scale, which is then treated as fa_kv_forward treats `scale`.  v_scale
 *             multiplies the normalised fp32 result once, in front of the store to o (in a key-split launch: behind the merge of the
 *             shares, whose partial outputs stay unscaled, so that a constant V is exact there too).
 *             LSE is that of the scaled scores and does not contain v_scale.  Consequence: whenever v_scale is a power of two the
 *             result is, bit for bit, v_scale x what fa_kv_forward gives on the cache dequantised to bf16 with scale' =
 *             fp32(scale * k_scale).  A V that is constant over the visible keys comes out as fp32(v_scale * that constant).
 *   dtypes    of q and o: FA_DTYPE_BF16 and FA_DTYPE_BF16_OUT_F32; FA_DTYPE_F32: FA_ERR_UNSUPPORTED.  d: 64 or 128.
 *   plan      that of the bf16 libraries: fa_kv8_splits_for and fa_kv8_workspace_bytes return what fa_kv_splits_for and
 *             fa_kv_workspace_bytes return for the same shapes (paged: bh_kv = batch * heads_kv).
 *
 * Out of scope: e5m2 and the fnuz encodings, per-head / per-token / block scales, an fp8 q or fp8 matrix instructions, a kernel
 * that quantises or appends rows.
 */
#ifndef FLASHATTN_AMD_KV8_H
#define FLASHATTN_AMD_KV8_H

#include "flashattn_amd_paged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLASHATTN_AMD_KV8_ABI_VERSION 1

/* Bytes of scratch a forward can use for these shapes (0: the plan does not split); paged: bh_kv = batch * heads_kv. */
size_t fa_kv8_workspace_bytes(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype);

/* Number of key shares S (1 .. 64) a call with a sufficient workspace runs with; 0 for rejected arguments. */
int32_t fa_kv8_splits_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype);

/* Name of the kernel family a forward launches for this call (page_size 0: the contiguous cache), or NULL for arguments it would reject. */
const char* fa_kv8_kernel_name_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                                   int32_t page_size);

/* The forward over a contiguous cache (bh_kv, capacity, d) of e4m3 bytes.  Enqueues one kernel (unsplit) or two on `stream` and returns. */
int fa_kv8_forward(const void* q, const void* k8, const void* v8, void* o, float* lse,
                   int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int64_t capacity, const int32_t* kv_lens,
                   int32_t d, float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype,
                   void* workspace, size_t workspace_bytes, void* stream);

/* The forward over a paged cache: the struct of flashattn_amd_paged.h, its pools read as e4m3 bytes. */
int fa_kv8_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse,
                         int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d,
                         float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Thread-local description of the last failure of an fa_kv8_* call on this thread ("" if none). */
const char* fa_kv8_last_error(void);

/* "flashattn_amd_kv8 abi <n> gfx950 ..." build string. */
const char* fa_kv8_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FLASHATTN_AMD_KV8_H */
