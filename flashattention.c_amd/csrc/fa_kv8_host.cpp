// fa_kv8_host.cpp -- the host side behind include/flashattn_amd_kv8.h: argument validation (no device is touched before it passes; lengths and
// the block table are device memory and never dereferenced here) and the entry points.  The checks are those of fa_kv_plan.cpp and
// fa_paged_host.cpp with an element of ONE byte; the plan is fa_kv.h's kv_plan: splits, share and workspace are what libflashattn_amd_kv.so
// reports for the same shapes.
#include "fa_kv8.h"
#include "flashattn_amd_kv8.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>

namespace fa {

static thread_local char g_kv8_error[320] = "";

static int kv8_fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_kv8_error, sizeof(g_kv8_error), fmt, ap);
    va_end(ap);
    return code;
}

// the shape part of the validation, shared by every entry point (contiguous: batch = bh_kv, heads_kv = 1)
static int check_shape(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t dtype)
{
    if (batch < 1 || heads_kv < 1 || group < 1 || nq < 1 || nk < 1) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "bh_kv (batch, heads_kv), group, nq and nk must be >= 1");
    if (dtype == FA_DTYPE_F32) return kv8_fail(FA_ERR_UNSUPPORTED, "FA_DTYPE_F32 is not supported: q and o are as in fa_kv_forward (FA_DTYPE_BF16, FA_DTYPE_BF16_OUT_F32)");
    if (dtype != FA_DTYPE_BF16 && dtype != FA_DTYPE_BF16_OUT_F32) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "unknown dtype %d", dtype);
    if (d != 64 && d != 128) return kv8_fail(FA_ERR_UNSUPPORTED, "head dim %d is not supported: 64 or 128", d);
    if (nk > (1 << 24)) return kv8_fail(FA_ERR_UNSUPPORTED, "nk = %lld exceeds 2^24", (long long)nk);
    if (nq > (1 << 30) || (int64_t)group * nq > (1 << 30)) return kv8_fail(FA_ERR_UNSUPPORTED, "group * nq exceeds 2^30");
    if (batch > 0x7fffffffLL || batch * heads_kv > 0x7fffffffLL || batch * heads_kv * group > 0x7fffffffLL)
        return kv8_fail(FA_ERR_UNSUPPORTED, "bh_kv * group (batch * heads_kv * group) exceeds 2^31 - 1");
    const int64_t bh_kv = batch * heads_kv;
    const KvPlan pl = kv_plan(bh_kv, group, nq, nk);
    if (bh_kv * pl.row_tiles * pl.splits > 0x7fffffffLL) return kv8_fail(FA_ERR_UNSUPPORTED, "the launch would exceed 2^31 - 1 workgroups");
    return FA_OK;
}

static int check_page_size(int32_t page_size)
{
    if (page_size < kPagedMinPage || page_size > kPagedMaxPage || (page_size & (page_size - 1)) != 0)
        return kv8_fail(FA_ERR_UNSUPPORTED, "page_size %d is not supported: a power of two, %d .. %d rows", page_size, kPagedMinPage, kPagedMaxPage);
    return FA_OK;
}

// scale' = fp32(scale * k_scale), the ONE product the contract names; v_scale
static int check_scales(float scale, float k_scale, float v_scale, float* folded)
{
    if (!std::isfinite(k_scale) || !(k_scale > 0.0f)) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "k_scale must be finite and > 0");
    if (!std::isfinite(v_scale) || !(v_scale > 0.0f)) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "v_scale must be finite and > 0");
    if (!std::isfinite(scale) || scale == 0.0f) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "scale must be finite and non-zero");
    const volatile float prod = scale * k_scale;   // volatile: rounded to fp32 here, whatever the host compiler's excess precision
    if (!std::isfinite(prod) || prod == 0.0f) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "scale * k_scale must be finite and non-zero in fp32");
    *folded = prod;
    return FA_OK;
}

static bool overlaps(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

// plan, parameters common to both entries, launch
static int run(Kv8Params& p8, const KvPlan& pl, size_t rows, int32_t d, float folded_scale, float v_scale, int32_t causal, int out_f32, int paged,
               void* workspace, void* stream)
{
    KvParams& p = p8.pg.kv;
    p.row_tiles = pl.row_tiles, p.splits = pl.splits, p.share = pl.share;
    p.scale_log2e = folded_scale * kLog2e;   // what fa_kv_plan.cpp does to `scale`
    p8.v_scale = v_scale;
    if (pl.splits > 1) {
        p.o_part = (float*)workspace;
        p.lse_part = p.o_part + (size_t)pl.splits * rows * d;
    }
    hipError_t e = launch_kv8_decode(p8, d, causal != 0, out_f32, paged, (hipStream_t)stream);
    if (e == hipSuccess && pl.splits > 1) e = launch_kv8_combine(p8, d, out_f32, (hipStream_t)stream);
    if (e != hipSuccess) return kv8_fail(e == hipErrorNoDevice ? FA_ERR_NO_DEVICE : FA_ERR_HIP, "launch failed: %s", hipGetErrorString(e));
    return FA_OK;
}

}  // namespace fa

using namespace fa;

extern "C" {

size_t fa_kv8_workspace_bytes(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype)
{
    (void)causal;
    if (check_shape(bh_kv, 1, group, nq, nk, d, dtype) != FA_OK) return 0;
    return kv_workspace_bytes(kv_plan(bh_kv, group, nq, nk), bh_kv, group, nq, d);
}

int32_t fa_kv8_splits_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype)
{
    (void)causal;
    if (check_shape(bh_kv, 1, group, nq, nk, d, dtype) != FA_OK) return 0;
    return kv_plan(bh_kv, group, nq, nk).splits;
}

const char* fa_kv8_kernel_name_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype, int32_t page_size)
{
    (void)causal;
    if (check_shape(bh_kv, 1, group, nq, nk, d, dtype) != FA_OK) return nullptr;
    if (page_size != 0 && check_page_size(page_size) != FA_OK) return nullptr;
    return kv8_decode_kernel_name();   // one family: paged or not is a template argument, the page size a launch parameter
}

int fa_kv8_forward(const void* q, const void* k8, const void* v8, void* o, float* lse, int64_t bh_kv, int32_t group, int64_t nq, int64_t nk,
                   int64_t capacity, const int32_t* kv_lens, int32_t d, float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype,
                   void* workspace, size_t workspace_bytes, void* stream)
{
    g_kv8_error[0] = 0;
    if (q == nullptr || k8 == nullptr || v8 == nullptr || o == nullptr) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "null pointer: q, k8, v8 and o are required");
    if (const int rc = check_shape(bh_kv, 1, group, nq, nk, d, dtype)) return rc;
    if (capacity < nk) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "nk = %lld exceeds capacity = %lld", (long long)nk, (long long)capacity);
    if ((uint64_t)capacity * (uint64_t)d >= (1ull << 32)) return kv8_fail(FA_ERR_UNSUPPORTED, "a K/V slab (capacity * d bytes) must stay below 2^32 bytes");
    float folded;
    if (const int rc = check_scales(scale, k_scale, v_scale, &folded)) return rc;
    if (((uintptr_t)q | (uintptr_t)k8 | (uintptr_t)v8 | (uintptr_t)o) & 15) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "q, k8, v8, o must be 16-byte aligned");
    if ((uintptr_t)lse & 3) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "lse must be 4-byte aligned");
    if ((uintptr_t)kv_lens & 3) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "kv_lens must be 4-byte aligned");
    if ((uintptr_t)workspace & 255) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "workspace must be 256-byte aligned");

    const int out_f32 = dtype == FA_DTYPE_BF16_OUT_F32;
    const size_t rows = (size_t)bh_kv * group * nq;
    const size_t q_bytes = rows * d * 2, o_bytes = rows * d * (out_f32 ? 4 : 2), kv_bytes = (size_t)bh_kv * capacity * d, lse_bytes = rows * 4;
    if (overlaps(o, o_bytes, q, q_bytes) || overlaps(o, o_bytes, k8, kv_bytes) || overlaps(o, o_bytes, v8, kv_bytes))
        return kv8_fail(FA_ERR_INVALID_ARGUMENT, "o overlaps q, k8 or v8 (k8 and v8 measured over their capacity)");
    if (lse != nullptr && (overlaps(lse, lse_bytes, q, q_bytes) || overlaps(lse, lse_bytes, k8, kv_bytes) || overlaps(lse, lse_bytes, v8, kv_bytes) ||
                           overlaps(lse, lse_bytes, o, o_bytes)))
        return kv8_fail(FA_ERR_INVALID_ARGUMENT, "lse overlaps q, k8, v8 or o");

    KvPlan pl = kv_plan(bh_kv, group, nq, nk);
    const size_t need = kv_workspace_bytes(pl, bh_kv, group, nq, d);
    if (workspace == nullptr || workspace_bytes == 0) {   // no scratch: the unsplit launch
        pl.splits = 1;
        pl.share = (int32_t)((nk + 63) / 64 * 64);
    } else {
        if (workspace_bytes < need)
            return kv8_fail(FA_ERR_INVALID_ARGUMENT, "workspace of %zu bytes is too small: fa_kv8_workspace_bytes() = %zu", workspace_bytes, need);
        const size_t ws = need ? need : 1;
        if (overlaps(workspace, ws, q, q_bytes) || overlaps(workspace, ws, k8, kv_bytes) || overlaps(workspace, ws, v8, kv_bytes) ||
            overlaps(workspace, ws, o, o_bytes) || (lse != nullptr && overlaps(workspace, ws, lse, lse_bytes)) ||
            (kv_lens != nullptr && overlaps(workspace, ws, kv_lens, (size_t)bh_kv * 4)))
            return kv8_fail(FA_ERR_INVALID_ARGUMENT, "the workspace overlaps a tensor of the call");
    }

    Kv8Params p8{};
    KvParams& p = p8.pg.kv;
    p.q = q, p.k = k8, p.v = v8, p.o = o, p.lse = lse, p.kv_lens = kv_lens;
    p.kv_slab_stride = capacity * d;
    p.m_rows = (int32_t)((int64_t)group * nq);
    p.nq = (int32_t)nq, p.nk = (int32_t)nk, p.bh_kv = (int32_t)bh_kv;
    return run(p8, pl, rows, d, folded, v_scale, causal, out_f32, 0, workspace, stream);
}

int fa_kv8_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse, int64_t batch, int32_t heads_kv, int32_t group, int64_t nq,
                         int64_t nk, int32_t d, float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype, void* workspace,
                         size_t workspace_bytes, void* stream)
{
    g_kv8_error[0] = 0;
    if (q == nullptr || cache == nullptr || o == nullptr) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "null pointer: q, cache and o are required");
    const fa_paged_cache& c = *cache;
    if (c.k_pool == nullptr || c.v_pool == nullptr || c.block_table == nullptr)
        return kv8_fail(FA_ERR_INVALID_ARGUMENT, "null pointer: k_pool, v_pool and block_table are required");
    if (const int rc = check_shape(batch, heads_kv, group, nq, nk, d, dtype)) return rc;
    if (const int rc = check_page_size(c.page_size)) return rc;
    if (c.num_pages < 1 || c.num_pages > 0x7fffffffLL) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "num_pages = %lld outside 1 .. 2^31 - 1", (long long)c.num_pages);
    if (c.max_pages < 1) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "max_pages must be >= 1");
    if (nk > (int64_t)c.max_pages * c.page_size)
        return kv8_fail(FA_ERR_INVALID_ARGUMENT, "nk = %lld exceeds max_pages * page_size = %lld", (long long)nk, (long long)c.max_pages * c.page_size);
    if ((c.page_stride | c.row_stride | c.head_stride) & 15)
        return kv8_fail(FA_ERR_INVALID_ARGUMENT, "page_stride, row_stride and head_stride must be multiples of 16 elements (16 bytes)");
    if (c.row_stride < d) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "row_stride = %lld is below d = %d", (long long)c.row_stride, d);
    if (c.page_stride < 1 || c.head_stride < 0) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "page_stride must be >= 1 and head_stride >= 0");
    if (c.page_stride > (1ll << 40) || c.head_stride > (1ll << 40) || c.row_stride > (1ll << 40))
        return kv8_fail(FA_ERR_UNSUPPORTED, "a stride exceeds 2^40 elements");
    // what a lane adds to a page base in 32 bits: the row inside the page and the head
    const uint64_t in_page = (uint64_t)c.page_size * (uint64_t)c.row_stride + (uint64_t)(heads_kv - 1) * (uint64_t)c.head_stride;
    if (in_page >= (1ull << 32))
        return kv8_fail(FA_ERR_UNSUPPORTED, "the offset inside a page (page_size * row_stride bytes plus the head offset = %llu) must stay below 2^32 bytes",
                        (unsigned long long)in_page);
    float folded;
    if (const int rc = check_scales(scale, k_scale, v_scale, &folded)) return rc;
    if (((uintptr_t)q | (uintptr_t)c.k_pool | (uintptr_t)c.v_pool | (uintptr_t)o) & 15)
        return kv8_fail(FA_ERR_INVALID_ARGUMENT, "q, k_pool, v_pool, o must be 16-byte aligned");
    if ((uintptr_t)lse & 3) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "lse must be 4-byte aligned");
    if (((uintptr_t)c.block_table | (uintptr_t)c.seq_lens) & 3) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "block_table and seq_lens must be 4-byte aligned");
    if ((uintptr_t)workspace & 255) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "workspace must be 256-byte aligned");

    const int out_f32 = dtype == FA_DTYPE_BF16_OUT_F32;
    const int64_t bh_kv = batch * heads_kv;
    const size_t rows = (size_t)bh_kv * group * nq;
    const size_t q_bytes = rows * d * 2, o_bytes = rows * d * (out_f32 ? 4 : 2), lse_bytes = rows * 4;
    // a pool over its whole strided extent: the last page's base, the last row of the last head in it, one row
    const size_t pool_bytes = (size_t)(c.num_pages - 1) * (size_t)c.page_stride + (size_t)(c.page_size - 1) * (size_t)c.row_stride +
                              (size_t)(heads_kv - 1) * (size_t)c.head_stride + (size_t)d;
    const size_t table_bytes = (size_t)batch * (size_t)c.max_pages * 4, lens_bytes = c.seq_lens != nullptr ? (size_t)batch * 4 : 0;
    auto hits_input = [&](const void* p, size_t n) {
        return overlaps(p, n, q, q_bytes) || overlaps(p, n, c.k_pool, pool_bytes) || overlaps(p, n, c.v_pool, pool_bytes) ||
               overlaps(p, n, c.block_table, table_bytes) || (lens_bytes != 0 && overlaps(p, n, c.seq_lens, lens_bytes));
    };
    if (hits_input(o, o_bytes)) return kv8_fail(FA_ERR_INVALID_ARGUMENT, "o overlaps q, a pool (measured over its whole strided extent), the block table or seq_lens");
    if (lse != nullptr && (hits_input(lse, lse_bytes) || overlaps(lse, lse_bytes, o, o_bytes)))
        return kv8_fail(FA_ERR_INVALID_ARGUMENT, "lse overlaps q, a pool, the block table, seq_lens or o");

    KvPlan pl = kv_plan(bh_kv, group, nq, nk);
    const size_t need = kv_workspace_bytes(pl, bh_kv, group, nq, d);
    if (workspace == nullptr || workspace_bytes == 0) {   // no scratch: the unsplit launch
        pl.splits = 1;
        pl.share = (int32_t)((nk + 63) / 64 * 64);
    } else {
        if (workspace_bytes < need)
            return kv8_fail(FA_ERR_INVALID_ARGUMENT, "workspace of %zu bytes is too small: fa_kv8_workspace_bytes() = %zu", workspace_bytes, need);
        const size_t ws = need ? need : 1;
        if (hits_input(workspace, ws) || overlaps(workspace, ws, o, o_bytes) || (lse != nullptr && overlaps(workspace, ws, lse, lse_bytes)))
            return kv8_fail(FA_ERR_INVALID_ARGUMENT, "the workspace overlaps a tensor of the call (pools over their whole extent, the block table)");
    }

    Kv8Params p8{};
    PagedParams& pp = p8.pg;
    KvParams& p = pp.kv;
    p.q = q, p.k = c.k_pool, p.v = c.v_pool, p.o = o, p.lse = lse, p.kv_lens = c.seq_lens;
    p.m_rows = (int32_t)((int64_t)group * nq);
    p.nq = (int32_t)nq, p.nk = (int32_t)nk, p.bh_kv = (int32_t)bh_kv;
    pp.table = c.block_table;
    pp.page_stride = c.page_stride, pp.head_stride = c.head_stride, pp.row_stride = (int32_t)c.row_stride;
    pp.max_pages = c.max_pages, pp.heads_kv = heads_kv;
    pp.page_shift = __builtin_ctz((unsigned)c.page_size);
    return run(p8, pl, rows, d, folded, v_scale, causal, out_f32, 1, workspace, stream);
}

const char* fa_kv8_last_error(void) { return g_kv8_error; }

const char* fa_kv8_version(void) { return "flashattn_amd_kv8 abi 1 gfx950 (K/V-cache attention over an fp8 e4m3fn cache, contiguous and paged)"; }

}  // extern "C"
