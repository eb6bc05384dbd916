// fa_kvw_host.cpp -- the entry points of include/flashattn_amd_kvw.h over fa_kv_host.h (validation, plan, launch parameters): those of
// fa_kv_plan.cpp and fa_paged_host.cpp plus the window, which the plan sees as the span of keys it is laid over (fa_kvw.h: kvw_span).
#include "fa_kv_host.h"
#include "fa_kvw.h"
#include "flashattn_amd_kvw.h"

namespace fa {

static thread_local KvError g_kvw_error;
static const KvWords kKvwWords = {2, "bh_kv", "caches are 16-bit", "bh_kv * group", "fa_kvw_workspace_bytes", "k", "v", "q, k, v, o"};
static const KvWords kKvwPagedWords = {2, "batch, heads_kv", "caches are 16-bit", "batch * heads_kv * group", "fa_kvw_paged_workspace_bytes", "k", "v", "q, k, v, o"};

// shape and window of a query (no pointers): the plan of the call, or nothing
static bool plan_query(const KvWords& words, int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t dtype,
                       int32_t window_left, KvPlan* pl)
{
    int32_t w;
    if (check_shape(g_kvw_error, words, batch, heads_kv, group, nq, nk, d, dtype) != FA_OK || check_window(g_kvw_error, window_left, &w) != FA_OK) return false;
    *pl = kv_plan(batch * heads_kv, group, nq, kvw_span(nq, nk, w));
    return true;
}

}  // namespace fa

using namespace fa;

extern "C" {

size_t fa_kvw_workspace_bytes(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype, int32_t window_left)
{
    (void)causal;
    KvPlan pl;
    if (!plan_query(kKvwWords, bh_kv, 1, group, nq, nk, d, dtype, window_left, &pl)) return 0;
    return kv_workspace_bytes(pl, bh_kv, group, nq, d);
}

int32_t fa_kvw_splits_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype, int32_t window_left)
{
    (void)causal;
    KvPlan pl;
    if (!plan_query(kKvwWords, bh_kv, 1, group, nq, nk, d, dtype, window_left, &pl)) return 0;
    return pl.splits;
}

const char* fa_kvw_kernel_name_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype, int32_t window_left)
{
    (void)causal;
    KvPlan pl;
    if (!plan_query(kKvwWords, bh_kv, 1, group, nq, nk, d, dtype, window_left, &pl)) return nullptr;
    return kvw_decode_kernel_name();
}

int fa_kvw_forward(const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh_kv, int32_t group, int64_t nq, int64_t nk,
                   int64_t capacity, const int32_t* kv_lens, int32_t d, float scale, int32_t causal, int32_t dtype, int32_t window_left,
                   void* workspace, size_t workspace_bytes, void* stream)
{
    KvError& e = g_kvw_error;
    e.text[0] = 0;
    const KvCall a = {q, o, lse, bh_kv, 1, group, nq, nk, d, dtype, workspace, workspace_bytes};
    if (const int rc = check_cache(e, kKvwWords, a, k, v, capacity)) return rc;
    if (const int rc = check_scale(e, scale)) return rc;
    KvwParams wp{};
    if (const int rc = check_window(e, window_left, &wp.window_left)) return rc;
    if (const int rc = plan_cache(e, kKvwWords, a, k, v, capacity, kv_lens, scale, wp.kv, kvw_span(nq, nk, wp.window_left))) return rc;
    hipError_t err = launch_kvw_decode(wp, d, causal != 0, a.out_f32(), (hipStream_t)stream);
    if (err == hipSuccess && wp.kv.splits > 1) err = launch_kv_combine(wp.kv, d, a.out_f32(), (hipStream_t)stream);
    return launch_result(e, err);
}

size_t fa_kvw_paged_workspace_bytes(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                                    int32_t window_left)
{
    (void)causal;
    KvPlan pl;
    if (!plan_query(kKvwPagedWords, batch, heads_kv, group, nq, nk, d, dtype, window_left, &pl)) return 0;
    return kv_workspace_bytes(pl, batch * heads_kv, group, nq, d);
}

int32_t fa_kvw_paged_splits_for(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                                int32_t window_left)
{
    (void)causal;
    KvPlan pl;
    if (!plan_query(kKvwPagedWords, batch, heads_kv, group, nq, nk, d, dtype, window_left, &pl)) return 0;
    return pl.splits;
}

int fa_kvw_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse, int64_t batch, int32_t heads_kv, int32_t group, int64_t nq,
                         int64_t nk, int32_t d, float scale, int32_t causal, int32_t dtype, int32_t window_left, void* workspace,
                         size_t workspace_bytes, void* stream)
{
    KvError& e = g_kvw_error;
    e.text[0] = 0;
    const KvCall a = {q, o, lse, batch, heads_kv, group, nq, nk, d, dtype, workspace, workspace_bytes};
    if (const int rc = check_pool(e, kKvwPagedWords, a, cache)) return rc;
    if (const int rc = check_scale(e, scale)) return rc;
    KvwPagedParams wp{};
    if (const int rc = check_window(e, window_left, &wp.window_left)) return rc;
    if (const int rc = plan_pool(e, kKvwPagedWords, a, *cache, scale, wp.pp, kvw_span(nq, nk, wp.window_left))) return rc;
    hipError_t err = launch_kvw_paged_decode(wp, d, causal != 0, a.out_f32(), (hipStream_t)stream);
    if (err == hipSuccess && wp.pp.kv.splits > 1) err = launch_kv_combine(wp.pp.kv, d, a.out_f32(), (hipStream_t)stream);
    return launch_result(e, err);
}

const char* fa_kvw_last_error(void) { return g_kvw_error.text; }

const char* fa_kvw_version(void) { return "flashattn_amd_kvw abi 1 gfx950 (sliding-window K/V-cache attention, contiguous and paged)"; }

}  // extern "C"
