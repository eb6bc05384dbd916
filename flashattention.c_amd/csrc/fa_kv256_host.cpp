// fa_kv256_host.cpp -- the entry points of include/flashattn_amd_kv256.h over fa_kv_host.h (validation, plan, launch parameters): those of
// fa_kvw_host.cpp at d = 256, with window_left = -1 for "no window" (the plan is then laid over nk, and the kernels without the window's selects run).
#include "fa_kv_host.h"
#include "fa_kv256.h"
#include "flashattn_amd_kv256.h"

namespace fa {

static thread_local KvError g_kv256_error;
static const KvWords kKv256Words = {2, "bh_kv", "caches are 16-bit", "bh_kv * group", "fa_kv256_workspace_bytes", "k", "v", "q, k, v, o"};
static const KvWords kKv256PagedWords = {2, "batch, heads_kv", "caches are 16-bit", "batch * heads_kv * group", "fa_kv256_paged_workspace_bytes", "k", "v", "q, k, v, o"};
static constexpr KvHeadDims kKv256Dims = {kKv256HeadDim, kKv256HeadDim};

// shape and window of a query (no pointers): the plan of the call, or nothing
static bool plan_query(const KvWords& words, int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t dtype,
                       int32_t window_left, KvPlan* pl)
{
    int32_t w;
    if (check_shape(g_kv256_error, words, batch, heads_kv, group, nq, nk, d, dtype, kKv256Dims) != FA_OK ||
        check_window_or_none(g_kv256_error, window_left, &w) != FA_OK)
        return false;
    *pl = kv_plan(batch * heads_kv, group, nq, w < 0 ? nk : kvw_span(nq, nk, w));
    return true;
}

}  // namespace fa

using namespace fa;

extern "C" {

size_t fa_kv256_workspace_bytes(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype, int32_t window_left)
{
    (void)causal;
    KvPlan pl;
    if (!plan_query(kKv256Words, bh_kv, 1, group, nq, nk, d, dtype, window_left, &pl)) return 0;
    return kv_workspace_bytes(pl, bh_kv, group, nq, d);
}

int32_t fa_kv256_splits_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype, int32_t window_left)
{
    (void)causal;
    KvPlan pl;
    if (!plan_query(kKv256Words, bh_kv, 1, group, nq, nk, d, dtype, window_left, &pl)) return 0;
    return pl.splits;
}

const char* fa_kv256_kernel_name_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype, int32_t window_left)
{
    (void)causal;
    KvPlan pl;
    if (!plan_query(kKv256Words, bh_kv, 1, group, nq, nk, d, dtype, window_left, &pl)) return nullptr;
    return kv256_decode_kernel_name();
}

int fa_kv256_forward(const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh_kv, int32_t group, int64_t nq, int64_t nk,
                     int64_t capacity, const int32_t* kv_lens, int32_t d, float scale, int32_t causal, int32_t dtype, int32_t window_left,
                     void* workspace, size_t workspace_bytes, void* stream)
{
    KvError& e = g_kv256_error;
    e.text[0] = 0;
    const KvCall a = {q, o, lse, bh_kv, 1, group, nq, nk, d, dtype, workspace, workspace_bytes};
    if (const int rc = check_cache(e, kKv256Words, a, k, v, capacity, kKv256Dims)) return rc;
    if (const int rc = check_scale(e, scale)) return rc;
    Kv256Params wp{};
    if (const int rc = check_window_or_none(e, window_left, &wp.window_left)) return rc;
    if (const int rc = plan_cache(e, kKv256Words, a, k, v, capacity, kv_lens, scale, wp.pp.kv, span_or_none(nq, nk, wp.window_left))) return rc;
    hipError_t err = launch_kv256_decode(wp, 0, wp.window_left >= 0, causal != 0, a.out_f32(), (hipStream_t)stream);
    if (err == hipSuccess && wp.pp.kv.splits > 1) err = launch_kv_combine(wp.pp.kv, d, a.out_f32(), (hipStream_t)stream);
    return launch_result(e, err);
}

size_t fa_kv256_paged_workspace_bytes(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                                      int32_t window_left)
{
    (void)causal;
    KvPlan pl;
    if (!plan_query(kKv256PagedWords, batch, heads_kv, group, nq, nk, d, dtype, window_left, &pl)) return 0;
    return kv_workspace_bytes(pl, batch * heads_kv, group, nq, d);
}

int32_t fa_kv256_paged_splits_for(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                                  int32_t window_left)
{
    (void)causal;
    KvPlan pl;
    if (!plan_query(kKv256PagedWords, batch, heads_kv, group, nq, nk, d, dtype, window_left, &pl)) return 0;
    return pl.splits;
}

int fa_kv256_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse, int64_t batch, int32_t heads_kv, int32_t group, int64_t nq,
                           int64_t nk, int32_t d, float scale, int32_t causal, int32_t dtype, int32_t window_left, void* workspace,
                           size_t workspace_bytes, void* stream)
{
    KvError& e = g_kv256_error;
    e.text[0] = 0;
    const KvCall a = {q, o, lse, batch, heads_kv, group, nq, nk, d, dtype, workspace, workspace_bytes};
    if (const int rc = check_pool(e, kKv256PagedWords, a, cache, kKv256Dims)) return rc;
    if (const int rc = check_scale(e, scale)) return rc;
    Kv256Params wp{};
    if (const int rc = check_window_or_none(e, window_left, &wp.window_left)) return rc;
    if (const int rc = plan_pool(e, kKv256PagedWords, a, *cache, scale, wp.pp, span_or_none(nq, nk, wp.window_left))) return rc;
    hipError_t err = launch_kv256_decode(wp, 1, wp.window_left >= 0, causal != 0, a.out_f32(), (hipStream_t)stream);
    if (err == hipSuccess && wp.pp.kv.splits > 1) err = launch_kv_combine(wp.pp.kv, d, a.out_f32(), (hipStream_t)stream);
    return launch_result(e, err);
}

const char* fa_kv256_last_error(void) { return g_kv256_error.text; }

const char* fa_kv256_version(void) { return "flashattn_amd_kv256 abi 1 gfx950 (K/V-cache attention at head dim 256: contiguous and paged, optional sliding window)"; }

}  // extern "C"
