// fa_kv_host.h -- the host side the KV-cache libraries share (fa_kv_plan.cpp, fa_paged_host.cpp, fa_kv8_host.cpp, fa_kvw_host.cpp, fa_kvw8_host.cpp): argument validation
// (no device is touched before it passes; lengths and block tables are device memory and never dereferenced here), the workspace and the
// plan it selects, and the fill of the launch parameters.  Inline, like kv_plan: the libraries link no host object of each other.  The plan
// is fa_kv.h's kv_plan over bh_kv = batch * heads_kv, so splits, share and workspace are the same in all of them for the same shapes (the windowed library: for the same span).
// Each library keeps its entry points, its version string and its own thread-local error text (KvError), and passes in the few words in
// which its messages differ (KvWords).  tests/test_kv_host_errors.py holds every check to its code and its text.
#pragma once
#include "fa_kvw.h"
#include "fa_paged.h"
#include "flashattn_amd_paged.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>

namespace fa {

struct KvError {
    char text[320] = "";
    int fail(int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)))
    {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(text, sizeof(text), fmt, ap);
        va_end(ap);
        return code;
    }
};

struct KvWords {
    int elem;                    // bytes per cache element: 2 (bf16) or 1 (e4m3)
    const char* slabs;           // how the library's shape arguments name the slab count
    const char* f32_why;         // what it says to FA_DTYPE_F32
    const char* slabs_x_group;   // ... and to too many query slabs
    const char* ws_fn;           // its function that reports the workspace size
    const char *k, *v;           // the contiguous entry's names of its caches ...
    const char* qkvo;            // ... and of its four 16-byte aligned tensors
};

// what every forward entry is given
struct KvCall {
    const void* q;
    void* o;
    float* lse;
    int64_t batch;      // contiguous cache: bh_kv, with heads_kv = 1
    int32_t heads_kv, group;
    int64_t nq, nk;
    int32_t d, dtype;
    void* workspace;
    size_t workspace_bytes;

    int64_t bh_kv() const { return batch * heads_kv; }
    int out_f32() const { return dtype == FA_DTYPE_BF16_OUT_F32; }
    size_t rows() const { return (size_t)bh_kv() * group * nq; }
    size_t q_bytes() const { return rows() * d * 2; }
    size_t o_bytes() const { return rows() * d * (out_f32() ? 4 : 2); }
    size_t lse_bytes() const { return rows() * 4; }
};

// the shape part of the validation, shared by every entry point and query
inline int check_shape(KvError& e, const KvWords& w, int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t dtype)
{
    if (batch < 1 || heads_kv < 1 || group < 1 || nq < 1 || nk < 1) return e.fail(FA_ERR_INVALID_ARGUMENT, "%s, group, nq and nk must be >= 1", w.slabs);
    if (dtype == FA_DTYPE_F32) return e.fail(FA_ERR_UNSUPPORTED, "FA_DTYPE_F32 is not supported: %s (FA_DTYPE_BF16, FA_DTYPE_BF16_OUT_F32)", w.f32_why);
    if (dtype != FA_DTYPE_BF16 && dtype != FA_DTYPE_BF16_OUT_F32) return e.fail(FA_ERR_INVALID_ARGUMENT, "unknown dtype %d", dtype);
    if (d != 64 && d != 128) return e.fail(FA_ERR_UNSUPPORTED, "head dim %d is not supported: 64 or 128", d);
    if (nk > (1 << 24)) return e.fail(FA_ERR_UNSUPPORTED, "nk = %lld exceeds 2^24", (long long)nk);
    if (nq > (1 << 30) || (int64_t)group * nq > (1 << 30)) return e.fail(FA_ERR_UNSUPPORTED, "group * nq exceeds 2^30");
    if (batch > 0x7fffffffLL || batch * heads_kv > 0x7fffffffLL || batch * heads_kv * group > 0x7fffffffLL)
        return e.fail(FA_ERR_UNSUPPORTED, "%s exceeds 2^31 - 1", w.slabs_x_group);
    const int64_t bh_kv = batch * heads_kv;
    const KvPlan pl = kv_plan(bh_kv, group, nq, nk);
    if (bh_kv * pl.row_tiles * pl.splits > 0x7fffffffLL) return e.fail(FA_ERR_UNSUPPORTED, "the launch would exceed 2^31 - 1 workgroups");
    return FA_OK;
}

inline int check_page_size(KvError& e, int32_t page_size)
{
    if (page_size < kPagedMinPage || page_size > kPagedMaxPage || (page_size & (page_size - 1)) != 0)
        return e.fail(FA_ERR_UNSUPPORTED, "page_size %d is not supported: a power of two, %d .. %d rows", page_size, kPagedMinPage, kPagedMaxPage);
    return FA_OK;
}

inline int check_scale(KvError& e, float scale)
{
    if (!std::isfinite(scale) || scale == 0.0f) return e.fail(FA_ERR_INVALID_ARGUMENT, "scale must be finite and non-zero");
    return FA_OK;
}

// the two scales of an fp8 cache (the libraries of fa_kv8.h and fa_kvw8.h): scale' = fp32(scale * k_scale), the ONE product the contract names; v_scale
inline int check_scales(KvError& e, float scale, float k_scale, float v_scale, float* folded)
{
    if (!std::isfinite(k_scale) || !(k_scale > 0.0f)) return e.fail(FA_ERR_INVALID_ARGUMENT, "k_scale must be finite and > 0");
    if (!std::isfinite(v_scale) || !(v_scale > 0.0f)) return e.fail(FA_ERR_INVALID_ARGUMENT, "v_scale must be finite and > 0");
    if (const int rc = check_scale(e, scale)) return rc;
    const volatile float prod = scale * k_scale;   // volatile: rounded to fp32 here, whatever the host compiler's excess precision
    if (!std::isfinite(prod) || prod == 0.0f) return e.fail(FA_ERR_INVALID_ARGUMENT, "scale * k_scale must be finite and non-zero in fp32");
    *folded = prod;
    return FA_OK;
}

// the window of a call (the libraries of fa_kvw.h and fa_kvw8.h): rejected below 0, saturated at 2^24 (no cache is longer)
inline int check_window(KvError& e, int32_t window_left, int32_t* w)
{
    if (window_left < 0) return e.fail(FA_ERR_INVALID_ARGUMENT, "window_left = %d must be >= 0", window_left);
    *w = window_left < kKvwMaxWindow ? window_left : kKvwMaxWindow;
    return FA_OK;
}

inline bool overlaps(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

// a slab of a contiguous cache: it holds the keys, and a lane's 32-bit offset reaches all of it
inline int check_capacity(KvError& e, const KvWords& w, int64_t nk, int32_t d, int64_t capacity)
{
    if (capacity < nk) return e.fail(FA_ERR_INVALID_ARGUMENT, "nk = %lld exceeds capacity = %lld", (long long)nk, (long long)capacity);
    if ((uint64_t)capacity * (uint64_t)d * (uint64_t)w.elem >= (1ull << 32))
        return e.fail(FA_ERR_UNSUPPORTED, "a K/V slab (capacity * d%s bytes) must stay below 2^32 bytes", w.elem == 2 ? " * 2" : "");
    return FA_OK;
}

// ---- a forward call in three steps, with the library's own checks of its scales between the first two ----
// 1 (contiguous cache): pointers, shape, the slab's extent
inline int check_cache(KvError& e, const KvWords& w, const KvCall& a, const void* k, const void* v, int64_t capacity)
{
    if (a.q == nullptr || k == nullptr || v == nullptr || a.o == nullptr)
        return e.fail(FA_ERR_INVALID_ARGUMENT, "null pointer: q, %s, %s and o are required", w.k, w.v);
    if (const int rc = check_shape(e, w, a.batch, a.heads_kv, a.group, a.nq, a.nk, a.d, a.dtype)) return rc;
    return check_capacity(e, w, a.nk, a.d, capacity);
}

// 1 (paged cache): pointers, shape, the geometry of the pool
inline int check_pool(KvError& e, const KvWords& w, const KvCall& a, const fa_paged_cache* cache)
{
    if (a.q == nullptr || cache == nullptr || a.o == nullptr) return e.fail(FA_ERR_INVALID_ARGUMENT, "null pointer: q, cache and o are required");
    const fa_paged_cache& c = *cache;
    if (c.k_pool == nullptr || c.v_pool == nullptr || c.block_table == nullptr)
        return e.fail(FA_ERR_INVALID_ARGUMENT, "null pointer: k_pool, v_pool and block_table are required");
    if (const int rc = check_shape(e, w, a.batch, a.heads_kv, a.group, a.nq, a.nk, a.d, a.dtype)) return rc;
    if (const int rc = check_page_size(e, c.page_size)) return rc;
    if (c.num_pages < 1 || c.num_pages > 0x7fffffffLL) return e.fail(FA_ERR_INVALID_ARGUMENT, "num_pages = %lld outside 1 .. 2^31 - 1", (long long)c.num_pages);
    if (c.max_pages < 1) return e.fail(FA_ERR_INVALID_ARGUMENT, "max_pages must be >= 1");
    if (a.nk > (int64_t)c.max_pages * c.page_size)
        return e.fail(FA_ERR_INVALID_ARGUMENT, "nk = %lld exceeds max_pages * page_size = %lld", (long long)a.nk, (long long)c.max_pages * c.page_size);
    if ((c.page_stride | c.row_stride | c.head_stride) & (16 / w.elem - 1))
        return e.fail(FA_ERR_INVALID_ARGUMENT, "page_stride, row_stride and head_stride must be multiples of %d elements (16 bytes)", 16 / w.elem);
    if (c.row_stride < a.d) return e.fail(FA_ERR_INVALID_ARGUMENT, "row_stride = %lld is below d = %d", (long long)c.row_stride, a.d);
    if (c.page_stride < 1 || c.head_stride < 0) return e.fail(FA_ERR_INVALID_ARGUMENT, "page_stride must be >= 1 and head_stride >= 0");
    if (c.page_stride > (1ll << 40) || c.head_stride > (1ll << 40) || c.row_stride > (1ll << 40))
        return e.fail(FA_ERR_UNSUPPORTED, "a stride exceeds 2^40 elements");
    // what a lane adds to a page base in 32 bits: the row inside the page and the head
    const uint64_t in_page = ((uint64_t)c.page_size * (uint64_t)c.row_stride + (uint64_t)(a.heads_kv - 1) * (uint64_t)c.head_stride) * (uint64_t)w.elem;
    if (in_page >= (1ull << 32))
        return e.fail(FA_ERR_UNSUPPORTED, "the offset inside a page (page_size * row_stride%s bytes plus the head offset = %llu) must stay below 2^32 bytes",
                      w.elem == 2 ? " * 2" : "", (unsigned long long)in_page);
    return FA_OK;
}

// alignment of everything the call names: four 16-byte pointers, lse, the int32 inputs (both pointers OR-ed), the workspace
inline int check_alignment(KvError& e, const KvCall& a, const void* k, const void* v, uintptr_t int32_inputs, const char* names16, const char* names4)
{
    if (((uintptr_t)a.q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)a.o) & 15) return e.fail(FA_ERR_INVALID_ARGUMENT, "%s must be 16-byte aligned", names16);
    if ((uintptr_t)a.lse & 3) return e.fail(FA_ERR_INVALID_ARGUMENT, "lse must be 4-byte aligned");
    if (int32_inputs & 3) return e.fail(FA_ERR_INVALID_ARGUMENT, "%s must be 4-byte aligned", names4);
    if ((uintptr_t)a.workspace & 255) return e.fail(FA_ERR_INVALID_ARGUMENT, "workspace must be 256-byte aligned");
    return FA_OK;
}

// The plan of the call -- unsplit where it comes without a workspace -- and how much of the workspace the kernels use (*ws: 0 without one,
// at least 1 with one, so that a workspace the plan does not need is still kept off the tensors).  span: the keys the plan is laid over --
// nk (0), or the widest key range of a row tile where a window bounds it from below (fa_kvw.h).
inline int plan_call(KvError& e, const KvWords& w, const KvCall& a, KvPlan& pl, size_t* ws, int64_t span = 0)
{
    if (span == 0) span = a.nk;
    pl = kv_plan(a.bh_kv(), a.group, a.nq, span);
    const size_t need = kv_workspace_bytes(pl, a.bh_kv(), a.group, a.nq, a.d);
    *ws = 0;
    if (a.workspace == nullptr || a.workspace_bytes == 0) {   // no scratch: the unsplit launch
        pl.splits = 1;
        pl.share = (int32_t)((span + 63) / 64 * 64);
        return FA_OK;
    }
    if (a.workspace_bytes < need)
        return e.fail(FA_ERR_INVALID_ARGUMENT, "workspace of %zu bytes is too small: %s() = %zu", a.workspace_bytes, w.ws_fn, need);
    *ws = need ? need : 1;
    return FA_OK;
}

// what every kernel takes (k, v, kv_lens and kv_slab_stride are the caller's)
inline void fill_params(const KvCall& a, const KvPlan& pl, float scale, KvParams& p)
{
    p.q = a.q, p.o = a.o, p.lse = a.lse;
    p.m_rows = (int32_t)((int64_t)a.group * a.nq);
    p.nq = (int32_t)a.nq, p.nk = (int32_t)a.nk, p.bh_kv = (int32_t)a.bh_kv();
    p.row_tiles = pl.row_tiles, p.splits = pl.splits, p.share = pl.share;
    p.scale_log2e = scale * kLog2e;
    if (pl.splits > 1) {
        p.o_part = (float*)a.workspace;
        p.lse_part = p.o_part + (size_t)pl.splits * a.rows() * a.d;
    }
}

// 2 (contiguous cache): alignment, overlap, workspace; then the launch parameters
inline int plan_cache(KvError& e, const KvWords& w, const KvCall& a, const void* k, const void* v, int64_t capacity, const int32_t* kv_lens, float scale,
                      KvParams& p, int64_t span = 0)
{
    if (const int rc = check_alignment(e, a, k, v, (uintptr_t)kv_lens, w.qkvo, "kv_lens")) return rc;
    const size_t q_bytes = a.q_bytes(), o_bytes = a.o_bytes(), lse_bytes = a.lse_bytes(), kv_bytes = (size_t)a.bh_kv() * capacity * a.d * w.elem;
    auto hits_input = [&](const void* x, size_t n) { return overlaps(x, n, a.q, q_bytes) || overlaps(x, n, k, kv_bytes) || overlaps(x, n, v, kv_bytes); };
    if (hits_input(a.o, o_bytes))
        return e.fail(FA_ERR_INVALID_ARGUMENT, "o overlaps q, %s or %s (%s and %s measured over their capacity)", w.k, w.v, w.k, w.v);
    if (a.lse != nullptr && (hits_input(a.lse, lse_bytes) || overlaps(a.lse, lse_bytes, a.o, o_bytes)))
        return e.fail(FA_ERR_INVALID_ARGUMENT, "lse overlaps q, %s, %s or o", w.k, w.v);
    KvPlan pl;
    size_t ws;
    if (const int rc = plan_call(e, w, a, pl, &ws, span)) return rc;
    if (ws != 0 && (hits_input(a.workspace, ws) || overlaps(a.workspace, ws, a.o, o_bytes) || (a.lse != nullptr && overlaps(a.workspace, ws, a.lse, lse_bytes)) ||
                    (kv_lens != nullptr && overlaps(a.workspace, ws, kv_lens, (size_t)a.bh_kv() * 4))))
        return e.fail(FA_ERR_INVALID_ARGUMENT, "the workspace overlaps a tensor of the call");
    fill_params(a, pl, scale, p);
    p.k = k, p.v = v, p.kv_lens = kv_lens;
    p.kv_slab_stride = capacity * a.d;
    return FA_OK;
}

// 2 (paged cache)
inline int plan_pool(KvError& e, const KvWords& w, const KvCall& a, const fa_paged_cache& c, float scale, PagedParams& pp, int64_t span = 0)
{
    if (const int rc = check_alignment(e, a, c.k_pool, c.v_pool, (uintptr_t)c.block_table | (uintptr_t)c.seq_lens, "q, k_pool, v_pool, o", "block_table and seq_lens"))
        return rc;
    const size_t q_bytes = a.q_bytes(), o_bytes = a.o_bytes(), lse_bytes = a.lse_bytes();
    // a pool over its whole strided extent: the last page's base, the last row of the last head in it, one row
    const size_t pool_bytes = ((size_t)(c.num_pages - 1) * (size_t)c.page_stride + (size_t)(c.page_size - 1) * (size_t)c.row_stride +
                               (size_t)(a.heads_kv - 1) * (size_t)c.head_stride + (size_t)a.d) * w.elem;
    const size_t table_bytes = (size_t)a.batch * (size_t)c.max_pages * 4, lens_bytes = c.seq_lens != nullptr ? (size_t)a.batch * 4 : 0;
    auto hits_input = [&](const void* x, size_t n) {
        return overlaps(x, n, a.q, q_bytes) || overlaps(x, n, c.k_pool, pool_bytes) || overlaps(x, n, c.v_pool, pool_bytes) ||
               overlaps(x, n, c.block_table, table_bytes) || (lens_bytes != 0 && overlaps(x, n, c.seq_lens, lens_bytes));
    };
    if (hits_input(a.o, o_bytes))
        return e.fail(FA_ERR_INVALID_ARGUMENT, "o overlaps q, a pool (measured over its whole strided extent), the block table or seq_lens");
    if (a.lse != nullptr && (hits_input(a.lse, lse_bytes) || overlaps(a.lse, lse_bytes, a.o, o_bytes)))
        return e.fail(FA_ERR_INVALID_ARGUMENT, "lse overlaps q, a pool, the block table, seq_lens or o");
    KvPlan pl;
    size_t ws;
    if (const int rc = plan_call(e, w, a, pl, &ws, span)) return rc;
    if (ws != 0 && (hits_input(a.workspace, ws) || overlaps(a.workspace, ws, a.o, o_bytes) || (a.lse != nullptr && overlaps(a.workspace, ws, a.lse, lse_bytes))))
        return e.fail(FA_ERR_INVALID_ARGUMENT, "the workspace overlaps a tensor of the call (pools over their whole extent, the block table)");
    fill_params(a, pl, scale, pp.kv);
    pp.kv.k = c.k_pool, pp.kv.v = c.v_pool, pp.kv.kv_lens = c.seq_lens;
    pp.table = c.block_table;
    pp.page_stride = c.page_stride, pp.head_stride = c.head_stride, pp.row_stride = (int32_t)c.row_stride;
    pp.max_pages = c.max_pages, pp.heads_kv = a.heads_kv;
    pp.page_shift = __builtin_ctz((unsigned)c.page_size);
    return FA_OK;
}

// 3: what a launch's hipError_t becomes
inline int launch_result(KvError& e, hipError_t err)
{
    if (err != hipSuccess) return e.fail(err == hipErrorNoDevice ? FA_ERR_NO_DEVICE : FA_ERR_HIP, "launch failed: %s", hipGetErrorString(err));
    return FA_OK;
}

}  // namespace fa
