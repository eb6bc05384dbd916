// fa_kv_plan.cpp -- the host side behind include/flashattn_amd_kv.h: argument validation (no device is touched before it passes),
// the plan (row tiles, key shares) and the entry points.  The reference has no such operator; the conventions are those of
// include/flashattn_amd.h.
#include "fa_kv.h"
#include "flashattn_amd_kv.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>

namespace fa {

static thread_local char g_kv_error[320] = "";

static int kv_fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_kv_error, sizeof(g_kv_error), fmt, ap);
    va_end(ap);
    return code;
}

// the shape part of the validation, shared by every entry point
static int check_shape(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t dtype)
{
    if (bh_kv < 1 || group < 1 || nq < 1 || nk < 1) return kv_fail(FA_ERR_INVALID_ARGUMENT, "bh_kv, group, nq and nk must be >= 1");
    if (dtype == FA_DTYPE_F32) return kv_fail(FA_ERR_UNSUPPORTED, "FA_DTYPE_F32 is not supported: caches are 16-bit (FA_DTYPE_BF16, FA_DTYPE_BF16_OUT_F32)");
    if (dtype != FA_DTYPE_BF16 && dtype != FA_DTYPE_BF16_OUT_F32) return kv_fail(FA_ERR_INVALID_ARGUMENT, "unknown dtype %d", dtype);
    if (d != 64 && d != 128) return kv_fail(FA_ERR_UNSUPPORTED, "head dim %d is not supported: 64 or 128", d);
    if (nk > (1 << 24)) return kv_fail(FA_ERR_UNSUPPORTED, "nk = %lld exceeds 2^24", (long long)nk);
    if (nq > (1 << 30) || (int64_t)group * nq > (1 << 30)) return kv_fail(FA_ERR_UNSUPPORTED, "group * nq exceeds 2^30");
    if (bh_kv > 0x7fffffffLL || bh_kv * group > 0x7fffffffLL) return kv_fail(FA_ERR_UNSUPPORTED, "bh_kv * group exceeds 2^31 - 1");
    const KvPlan pl = kv_plan(bh_kv, group, nq, nk);
    if (bh_kv * pl.row_tiles * pl.splits > 0x7fffffffLL) return kv_fail(FA_ERR_UNSUPPORTED, "the launch would exceed 2^31 - 1 workgroups");
    return FA_OK;
}

static bool overlaps(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace fa

using namespace fa;

extern "C" {

size_t fa_kv_workspace_bytes(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype)
{
    (void)causal;
    if (check_shape(bh_kv, group, nq, nk, d, dtype) != FA_OK) return 0;
    return kv_workspace_bytes(kv_plan(bh_kv, group, nq, nk), bh_kv, group, nq, d);
}

int32_t fa_kv_splits_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype)
{
    (void)causal;
    if (check_shape(bh_kv, group, nq, nk, d, dtype) != FA_OK) return 0;
    return kv_plan(bh_kv, group, nq, nk).splits;
}

const char* fa_kv_kernel_name_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype)
{
    (void)causal;
    if (check_shape(bh_kv, group, nq, nk, d, dtype) != FA_OK) return nullptr;
    return kv_decode_kernel_name();
}

int fa_kv_forward(const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh_kv, int32_t group, int64_t nq, int64_t nk,
                  int64_t capacity, const int32_t* kv_lens, int32_t d, float scale, int32_t causal, int32_t dtype, void* workspace,
                  size_t workspace_bytes, void* stream)
{
    g_kv_error[0] = 0;
    if (q == nullptr || k == nullptr || v == nullptr || o == nullptr) return kv_fail(FA_ERR_INVALID_ARGUMENT, "null pointer: q, k, v and o are required");
    if (const int rc = check_shape(bh_kv, group, nq, nk, d, dtype)) return rc;
    if (capacity < nk) return kv_fail(FA_ERR_INVALID_ARGUMENT, "nk = %lld exceeds capacity = %lld", (long long)nk, (long long)capacity);
    if ((uint64_t)capacity * (uint64_t)d * 2u >= (1ull << 32)) return kv_fail(FA_ERR_UNSUPPORTED, "a K/V slab (capacity * d * 2 bytes) must stay below 2^32 bytes");
    if (!(std::isfinite(scale)) || scale == 0.0f) return kv_fail(FA_ERR_INVALID_ARGUMENT, "scale must be finite and non-zero");
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15) return kv_fail(FA_ERR_INVALID_ARGUMENT, "q, k, v, o must be 16-byte aligned");
    if ((uintptr_t)lse & 3) return kv_fail(FA_ERR_INVALID_ARGUMENT, "lse must be 4-byte aligned");
    if ((uintptr_t)kv_lens & 3) return kv_fail(FA_ERR_INVALID_ARGUMENT, "kv_lens must be 4-byte aligned");
    if ((uintptr_t)workspace & 255) return kv_fail(FA_ERR_INVALID_ARGUMENT, "workspace must be 256-byte aligned");

    const int out_f32 = dtype == FA_DTYPE_BF16_OUT_F32;
    const size_t rows = (size_t)bh_kv * group * nq;
    const size_t q_bytes = rows * d * 2, o_bytes = rows * d * (out_f32 ? 4 : 2), kv_bytes = (size_t)bh_kv * capacity * d * 2, lse_bytes = rows * 4;
    if (overlaps(o, o_bytes, q, q_bytes) || overlaps(o, o_bytes, k, kv_bytes) || overlaps(o, o_bytes, v, kv_bytes))
        return kv_fail(FA_ERR_INVALID_ARGUMENT, "o overlaps q, k or v (k and v measured over their capacity)");
    if (lse != nullptr && (overlaps(lse, lse_bytes, q, q_bytes) || overlaps(lse, lse_bytes, k, kv_bytes) || overlaps(lse, lse_bytes, v, kv_bytes) ||
                           overlaps(lse, lse_bytes, o, o_bytes)))
        return kv_fail(FA_ERR_INVALID_ARGUMENT, "lse overlaps q, k, v or o");

    KvPlan pl = kv_plan(bh_kv, group, nq, nk);
    const size_t need = kv_workspace_bytes(pl, bh_kv, group, nq, d);
    if (workspace == nullptr || workspace_bytes == 0) {   // no scratch: the unsplit launch
        pl.splits = 1;
        pl.share = (int32_t)((nk + 63) / 64 * 64);
    } else {
        if (workspace_bytes < need)
            return kv_fail(FA_ERR_INVALID_ARGUMENT, "workspace of %zu bytes is too small: fa_kv_workspace_bytes() = %zu", workspace_bytes, need);
        const size_t ws = need ? need : 1;
        if (overlaps(workspace, ws, q, q_bytes) || overlaps(workspace, ws, k, kv_bytes) || overlaps(workspace, ws, v, kv_bytes) ||
            overlaps(workspace, ws, o, o_bytes) || (lse != nullptr && overlaps(workspace, ws, lse, lse_bytes)) ||
            (kv_lens != nullptr && overlaps(workspace, ws, kv_lens, (size_t)bh_kv * 4)))
            return kv_fail(FA_ERR_INVALID_ARGUMENT, "the workspace overlaps a tensor of the call");
    }

    KvParams p{};
    p.q = q, p.k = k, p.v = v, p.o = o, p.lse = lse, p.kv_lens = kv_lens;
    p.kv_slab_stride = capacity * d;
    p.m_rows = (int32_t)((int64_t)group * nq);
    p.nq = (int32_t)nq, p.nk = (int32_t)nk, p.bh_kv = (int32_t)bh_kv;
    p.row_tiles = pl.row_tiles, p.splits = pl.splits, p.share = pl.share;
    p.scale_log2e = scale * kLog2e;
    if (pl.splits > 1) {
        p.o_part = (float*)workspace;
        p.lse_part = p.o_part + (size_t)pl.splits * rows * d;
    }
    hipError_t e = launch_kv_decode(p, d, causal != 0, out_f32, (hipStream_t)stream);
    if (e == hipSuccess && pl.splits > 1) e = launch_kv_combine(p, d, out_f32, (hipStream_t)stream);
    if (e != hipSuccess) return kv_fail(e == hipErrorNoDevice ? FA_ERR_NO_DEVICE : FA_ERR_HIP, "launch failed: %s", hipGetErrorString(e));
    return FA_OK;
}

int fa_kv_stream_read(const void* k, const void* v, int64_t bh_kv, int64_t nk, int64_t capacity, int32_t d, void* sink, void* stream)
{
    g_kv_error[0] = 0;
    if (k == nullptr || v == nullptr || sink == nullptr) return kv_fail(FA_ERR_INVALID_ARGUMENT, "null pointer: k, v and sink are required");
    if (const int rc = check_shape(bh_kv, 1, 1, nk, d, FA_DTYPE_BF16)) return rc;
    if (capacity < nk) return kv_fail(FA_ERR_INVALID_ARGUMENT, "nk = %lld exceeds capacity = %lld", (long long)nk, (long long)capacity);
    if ((uint64_t)capacity * (uint64_t)d * 2u >= (1ull << 32)) return kv_fail(FA_ERR_UNSUPPORTED, "a K/V slab (capacity * d * 2 bytes) must stay below 2^32 bytes");
    if (((uintptr_t)k | (uintptr_t)v | (uintptr_t)sink) & 15) return kv_fail(FA_ERR_INVALID_ARGUMENT, "k, v, sink must be 16-byte aligned");
    const hipError_t e = launch_kv_stream_read(k, v, bh_kv, nk, capacity, d, kv_plan(bh_kv, 1, 1, nk), (uint32_t*)sink, (hipStream_t)stream);
    if (e != hipSuccess) return kv_fail(e == hipErrorNoDevice ? FA_ERR_NO_DEVICE : FA_ERR_HIP, "launch failed: %s", hipGetErrorString(e));
    return FA_OK;
}

const char* fa_kv_last_error(void) { return g_kv_error; }

const char* fa_kv_version(void) { return "flashattn_amd_kv abi 1 gfx950 (K/V-cache attention: nq != nk, GQA, split-key decode)"; }

}  // extern "C"
