// fa_kvw8_host.cpp -- the entry points of include/flashattn_amd_kvw8.h over fa_kv_host.h (validation, plan, launch parameters): those of
// fa_kv8_host.cpp (an element of ONE byte, the two scales of the cache) plus the window of fa_kvw_host.cpp, which the plan sees as the span of
// keys it is laid over (fa_kvw.h: kvw_span).
#include "fa_kv_host.h"
#include "fa_kvw8.h"
#include "flashattn_amd_kvw8.h"

namespace fa {

static thread_local KvError g_kvw8_error;
static const KvWords kKvw8Words = {1, "bh_kv", "q and o are as in fa_kv_forward", "bh_kv * group", "fa_kvw8_workspace_bytes", "k8", "v8", "q, k8, v8, o"};
static const KvWords kKvw8PagedWords = {1, "batch, heads_kv", "q and o are as in fa_kv_forward", "batch * heads_kv * group", "fa_kvw8_paged_workspace_bytes",
                                        "k8", "v8", "q, k8, v8, o"};

// shape and window of a query (no pointers): the plan of the call, or nothing
static bool plan_query(const KvWords& words, int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t dtype,
                       int32_t window_left, KvPlan* pl)
{
    int32_t w;
    if (check_shape(g_kvw8_error, words, batch, heads_kv, group, nq, nk, d, dtype) != FA_OK || check_window(g_kvw8_error, window_left, &w) != FA_OK) return false;
    *pl = kv_plan(batch * heads_kv, group, nq, kvw_span(nq, nk, w));
    return true;
}

static int run(KvError& e, Kvw8Params& wp, int32_t d, float v_scale, int32_t causal, int out_f32, int paged, void* stream)
{
    wp.k8.v_scale = v_scale;
    hipError_t err = launch_kvw8_decode(wp, d, causal != 0, out_f32, paged, (hipStream_t)stream);
    if (err == hipSuccess && wp.k8.pg.kv.splits > 1) err = launch_kv8_combine(wp.k8, d, out_f32, (hipStream_t)stream);
    return launch_result(e, err);
}

}  // namespace fa

using namespace fa;

extern "C" {

size_t fa_kvw8_workspace_bytes(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype, int32_t window_left)
{
    (void)causal;
    KvPlan pl;
    if (!plan_query(kKvw8Words, bh_kv, 1, group, nq, nk, d, dtype, window_left, &pl)) return 0;
    return kv_workspace_bytes(pl, bh_kv, group, nq, d);
}

int32_t fa_kvw8_splits_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype, int32_t window_left)
{
    (void)causal;
    KvPlan pl;
    if (!plan_query(kKvw8Words, bh_kv, 1, group, nq, nk, d, dtype, window_left, &pl)) return 0;
    return pl.splits;
}

const char* fa_kvw8_kernel_name_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype, int32_t page_size,
                                    int32_t window_left)
{
    (void)causal;
    KvPlan pl;
    if (!plan_query(kKvw8Words, bh_kv, 1, group, nq, nk, d, dtype, window_left, &pl)) return nullptr;
    if (page_size != 0 && check_page_size(g_kvw8_error, page_size) != FA_OK) return nullptr;
    return kvw8_decode_kernel_name();   // one family: paged or not is a template argument, the page size a launch parameter
}

int fa_kvw8_forward(const void* q, const void* k8, const void* v8, void* o, float* lse, int64_t bh_kv, int32_t group, int64_t nq, int64_t nk,
                    int64_t capacity, const int32_t* kv_lens, int32_t d, float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype,
                    int32_t window_left, void* workspace, size_t workspace_bytes, void* stream)
{
    KvError& e = g_kvw8_error;
    e.text[0] = 0;
    const KvCall a = {q, o, lse, bh_kv, 1, group, nq, nk, d, dtype, workspace, workspace_bytes};
    if (const int rc = check_cache(e, kKvw8Words, a, k8, v8, capacity)) return rc;
    float folded;
    if (const int rc = check_scales(e, scale, k_scale, v_scale, &folded)) return rc;
    Kvw8Params wp{};
    if (const int rc = check_window(e, window_left, &wp.window_left)) return rc;
    if (const int rc = plan_cache(e, kKvw8Words, a, k8, v8, capacity, kv_lens, folded, wp.k8.pg.kv, kvw_span(nq, nk, wp.window_left))) return rc;
    return run(e, wp, d, v_scale, causal, a.out_f32(), 0, stream);
}

size_t fa_kvw8_paged_workspace_bytes(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                                     int32_t window_left)
{
    (void)causal;
    KvPlan pl;
    if (!plan_query(kKvw8PagedWords, batch, heads_kv, group, nq, nk, d, dtype, window_left, &pl)) return 0;
    return kv_workspace_bytes(pl, batch * heads_kv, group, nq, d);
}

int32_t fa_kvw8_paged_splits_for(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                                 int32_t window_left)
{
    (void)causal;
    KvPlan pl;
    if (!plan_query(kKvw8PagedWords, batch, heads_kv, group, nq, nk, d, dtype, window_left, &pl)) return 0;
    return pl.splits;
}

int fa_kvw8_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse, int64_t batch, int32_t heads_kv, int32_t group, int64_t nq,
                          int64_t nk, int32_t d, float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype, int32_t window_left,
                          void* workspace, size_t workspace_bytes, void* stream)
{
    KvError& e = g_kvw8_error;
    e.text[0] = 0;
    const KvCall a = {q, o, lse, batch, heads_kv, group, nq, nk, d, dtype, workspace, workspace_bytes};
    if (const int rc = check_pool(e, kKvw8PagedWords, a, cache)) return rc;
    float folded;
    if (const int rc = check_scales(e, scale, k_scale, v_scale, &folded)) return rc;
    Kvw8Params wp{};
    if (const int rc = check_window(e, window_left, &wp.window_left)) return rc;
    if (const int rc = plan_pool(e, kKvw8PagedWords, a, *cache, folded, wp.k8.pg, kvw_span(nq, nk, wp.window_left))) return rc;
    return run(e, wp, d, v_scale, causal, a.out_f32(), 1, stream);
}

const char* fa_kvw8_last_error(void) { return g_kvw8_error.text; }

const char* fa_kvw8_version(void) { return "flashattn_amd_kvw8 abi 1 gfx950 (sliding-window K/V-cache attention over an fp8 e4m3fn cache, contiguous and paged)"; }

}  // extern "C"
