/*
 * include/flashattn_amd_kv.h -- C ABI of the KV-cache attention extension (libflashattn_amd_kv.so), beside the frozen
 *                               include/flashattn_amd.h (ABI 6), whose status codes and dtypes it shares.
 *
 * Few query rows against many cached keys: decode (1 .. 16 new tokens), chunked prefill, cross-attention, and grouped-query
 * attention (several query heads share one K/V head).  The square entries of the main header cannot express nq != nk.
 *
 * Conventions are the main header's: plain C, raw device pointers, an opaque HIP stream, fa_status return codes, a
 * thread-local error text (fa_kv_last_error), no allocation, no synchronisation, legal while `stream` is capturing.
 *
 * Semantics
 *   tensors   q, o : (bh_kv * group, nq, d) row-major contiguous; slab index = kv_slab * group + g
 *             k, v : (bh_kv, capacity, d); only rows [0, len) of a slab are ever read -- rows [len, capacity) and the
 *                    other slabs are never touched
 *             lse  : NULL or (bh_kv * group, nq) fp32, natural log
 *             kv_lens : NULL (every slab has len = nk) or a DEVICE pointer to int32[bh_kv]; each value is clamped to
 *                    [0, nk].  It is read on the device only -- the host never dereferences it -- so one captured graph
 *                    can be replayed while the cache grows.
 *   math      O = softmax(scale * q K^T) V per query slab, over the first `len` keys of its K/V slab
 *   causal    bottom-right aligned: query row i sees keys j <= len - nq + i (a cache that holds the new tokens' keys at
 *             its end); per slab when kv_lens is given
 *   no keys   rows with no visible key (len = 0, or causal with len < nq) get O = 0 and LSE = -inf, never NaN
 *   dtypes    FA_DTYPE_BF16 (bf16 in, bf16 out) and FA_DTYPE_BF16_OUT_F32 (bf16 in, fp32 out).  FA_DTYPE_F32:
 *             FA_ERR_UNSUPPORTED (caches are 16-bit)
 *   d         64 or 128; anything else: FA_ERR_UNSUPPORTED
 *   arithmetic  one form for both dtypes: Q.K^T is one bf16 product in an fp32 accumulator; P is bf16 hi + bf16 lo (lo =
 *             the bf16 of the exact residual); V as it is; fp32 accumulators.  Accuracy: what the main header states for
 *             FA_DTYPE_BF16_OUT_F32 (weights to 2^-17; <= 2e-4 on every data family tested); a bf16 output adds its own
 *             single rounding.  A V that is constant over the visible keys comes out exactly.
 *   capacity  capacity >= nk; a slab must stay below 2^32 bytes (capacity * d * 2), larger: FA_ERR_UNSUPPORTED
 *   ranges    nq, nk >= 1; nk <= 2^24; group >= 1; group * nq <= 2^30; bh_kv * group <= 2^31 - 1
 *   alignment q, k, v, o 16 bytes; lse 4; workspace 256
 *   overlap   o must overlap none of q, k, v; the workspace must overlap no tensor of the call (k, v measured over their
 *             whole capacity): FA_ERR_INVALID_ARGUMENT
 *   workspace caller-owned scratch of a key-split launch (normalised fp32 partial outputs and their log-sum-exps, one set
 *             per key share).  fa_kv_workspace_bytes depends on the shapes only, never on kv_lens; it is 0 when the plan does
 *             not split and for arguments fa_kv_forward would reject.  NULL or 0 bytes: the call runs unsplit.  Non-NULL
 *             but smaller than fa_kv_workspace_bytes: FA_ERR_INVALID_ARGUMENT.  Contents need no initialisation.
 */
#ifndef FLASHATTN_AMD_KV_H
#define FLASHATTN_AMD_KV_H

#include "flashattn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLASHATTN_AMD_KV_ABI_VERSION 1

/* Bytes of scratch fa_kv_forward can use for these shapes (0: the plan does not split). */
size_t fa_kv_workspace_bytes(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype);

/* Number of key shares S (1 .. 64) a call with a sufficient workspace runs with; 0 for rejected arguments. */
int32_t fa_kv_splits_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype);

/* The forward.  Enqueues one kernel (unsplit) or two (key shares + combine) on `stream` and returns. */
int fa_kv_forward(const void* q, const void* k, const void* v, void* o, float* lse,
                  int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int64_t capacity, const int32_t* kv_lens,
                  int32_t d, float scale, int32_t causal, int32_t dtype,
                  void* workspace, size_t workspace_bytes, void* stream);

/*
 * Measurement aid: reads exactly the K/V bytes fa_kv_forward needs -- rows [0, nk) of every slab -- with 16-byte loads
 * on the grid of a one-row-tile forward, and folds them with XOR into one word per workgroup of `sink` (device, at
 * least 4 KiB, 16-byte aligned).  The bandwidth floor of the forward on the same buffers.  bf16 caches, d 64 or 128.
 */
int fa_kv_stream_read(const void* k, const void* v, int64_t bh_kv, int64_t nk, int64_t capacity, int32_t d,
                      void* sink, void* stream);

/* Name of the kernel family fa_kv_forward launches for this call, or NULL for arguments it would reject. */
const char* fa_kv_kernel_name_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype);

/* Thread-local description of the last failure of an fa_kv_* call on this thread ("" if none). */
const char* fa_kv_last_error(void);

/* "flashattn_amd_kv abi <n> gfx950 ..." build string. */
const char* fa_kv_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FLASHATTN_AMD_KV_H */
