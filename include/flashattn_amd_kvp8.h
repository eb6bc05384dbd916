/*
 * include/flashattn_amd_kvp8.h -- C ABI of chunked prefill over the fp8 (e4m3fn) K/V caches (libflashattn_amd_kvp8.so), beside
 *                                 include/flashattn_amd_kvp.h (the same calls over bf16 caches), whose semantics it keeps, and
 *                                 include/flashattn_amd_kv8.h (the decode kernels over the same caches), whose cache and scales
 *                                 it keeps.  Status codes and dtypes are those of the frozen include/flashattn_amd.h (ABI 6).
 *
 * fa_kv8_forward and fa_kv8_paged_forward run a decode kernel: a workgroup owns 32 packed query rows and streams -- and converts --
 * the whole K/V slab for them, group * nq / 32 times per slab for a chunk of nq rows.  fa_kvp8_forward and fa_kvp8_paged_forward
 * are the same two calls on the chunked-prefill kernel of include/flashattn_amd_kvp.h: a workgroup owns 256 packed rows, and every
 * 64-key block is loaded, converted to bf16 and written to LDS once per workgroup (docs/kv_prefill_fp8.md has the design and the
 * measurements).  There is no key split: the calls take no workspace.
 *
 * Conventions are the main header's: plain C, raw device pointers, an opaque HIP stream, fa_status return codes, a thread-local
 * error text (fa_kvp8_last_error), no allocation, no synchronisation, legal while `stream` is capturing; nothing on the device
 * is touched before validation passes.  kv_lens / seq_lens and the block table are read on the device only.
 *
 * Semantics
 *   everything include/flashattn_amd_kvp.h says carries over: d = 128 only ("head dim 64 is not supported: 128"), FA_DTYPE_BF16 and
 *             FA_DTYPE_BF16_OUT_F32 for q and o, packed rows (bh_kv * group, nq, d), GQA, bottom-right aligned causal masking
 *             (j <= len - nq + i), rows without a visible key (O = 0, LSE = -inf, never NaN), no K/V row at or beyond len and no
 *             block-table entry at or beyond ceil(len / page_size) read, loads past the last visible row redirected to it on the
 *             logical row and before the table lookup.
 *   the cache is that of include/flashattn_amd_kv8.h: one OCP e4m3fn byte per element, strides in elements = bytes, 16-byte
 *             alignment, paged strides multiples of 16 elements, a slab (capacity * d bytes) and the offset inside a page below
 *             2^32 bytes.  Rows that are never read may hold anything, the NaN codes 0x7F / 0xFF included.
 *   scales    k_scale and v_scale are host floats, finite and > 0: logical K = k_scale x the stored values, logical V = v_scale x
 *             them.  scale' = fp32(scale * k_scale) is formed on the host as ONE fp32 product and must be finite and non-zero;
 *             v_scale multiplies the normalised fp32 result once, in front of the store.  The LSE is that of the scaled scores:
 *             it does not contain v_scale.
 *   contract  e4m3 -> bf16 is exact, and the kernel runs the instruction sequence of fa_kvp_forward on the converted values.  With
 *             v_scale a power of two the result is, bit for bit, v_scale x what fa_kvp_forward gives on the cache dequantised to
 *             bf16 at scale'; the LSE is bit-equal to fa_kvp_forward's for any v_scale; fa_kvp8_paged_forward equals
 *             fa_kvp8_forward on the gathered bytes, bit for bit; a V that is constant over the visible keys comes out as
 *             fp32(v_scale * constant).
 *
 * window_left is served by include/flashattn_amd_kvpw.h (libflashattn_amd_kvpw.so).
 * Out of scope: head dims 64 and 256, a key split for grids of a few workgroups, and routing from fa_kv8_forward /
 * fa_kv8_paged_forward, which keep their kernels and their bits.
 */
#ifndef FLASHATTN_AMD_KVP8_H
#define FLASHATTN_AMD_KVP8_H

#include "flashattn_amd.h"
#include "flashattn_amd_paged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLASHATTN_AMD_KVP8_ABI_VERSION 1

/* Name of the kernel family fa_kvp8_forward launches for this call, or NULL for arguments it would reject. */
const char* fa_kvp8_kernel_name_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype);

/* Enqueues one kernel on `stream` and returns.  The arguments are fa_kv8_forward's without the workspace. */
int fa_kvp8_forward(const void* q, const void* k8, const void* v8, void* o, float* lse,
                    int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int64_t capacity, const int32_t* kv_lens,
                    int32_t d, float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype, void* stream);

/* The same for a paged cache: fa_kv8_paged_forward's arguments without the workspace. */
int fa_kvp8_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse,
                          int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d,
                          float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype, void* stream);

/* Thread-local description of the last failure of an fa_kvp8_* call on this thread ("" if none). */
const char* fa_kvp8_last_error(void);

/* "flashattn_amd_kvp8 abi <n> gfx950 ..." build string. */
const char* fa_kvp8_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FLASHATTN_AMD_KVP8_H */
