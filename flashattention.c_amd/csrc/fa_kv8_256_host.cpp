// fa_kv8_256_host.cpp -- the entry points of include/flashattn_amd_kv8_256.h over fa_kv_host.h (validation, plan, launch parameters): those of
// fa_kv256_host.cpp (d = 256, window_left = -1 for "no window") over a cache of ONE byte per element with the two scales of fa_kvw8_host.cpp.
#include "fa_kv_host.h"
#include "fa_kv8_256.h"
#include "flashattn_amd_kv8_256.h"

namespace fa {

static thread_local KvError g_kv8_256_error;
static const KvWords kKv8x256Words = {1, "bh_kv", "q and o are as in fa_kv_forward", "bh_kv * group", "fa_kv8_256_workspace_bytes", "k8", "v8", "q, k8, v8, o"};
static const KvWords kKv8x256PagedWords = {1, "batch, heads_kv", "q and o are as in fa_kv_forward", "batch * heads_kv * group",
                                           "fa_kv8_256_paged_workspace_bytes", "k8", "v8", "q, k8, v8, o"};
static constexpr KvHeadDims kKv8x256Dims = {kKv256HeadDim, kKv256HeadDim};

// shape and window of a query (no pointers): the plan of the call, or nothing
static bool plan_query(const KvWords& words, int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t dtype,
                       int32_t window_left, KvPlan* pl)
{
    int32_t w;
    if (check_shape(g_kv8_256_error, words, batch, heads_kv, group, nq, nk, d, dtype, kKv8x256Dims) != FA_OK ||
        check_window_or_none(g_kv8_256_error, window_left, &w) != FA_OK)
        return false;
    *pl = kv_plan(batch * heads_kv, group, nq, w < 0 ? nk : kvw_span(nq, nk, w));
    return true;
}

static int run(KvError& e, Kv8x256Params& wp, int32_t d, float v_scale, int32_t causal, int out_f32, int paged, void* stream)
{
    wp.k8.v_scale = v_scale;
    hipError_t err = launch_kv8_256_decode(wp, paged, wp.window_left >= 0, causal != 0, out_f32, (hipStream_t)stream);
    if (err == hipSuccess && wp.k8.pg.kv.splits > 1) err = launch_kv8_combine(wp.k8, d, out_f32, (hipStream_t)stream);
    return launch_result(e, err);
}

}  // namespace fa

using namespace fa;

extern "C" {

size_t fa_kv8_256_workspace_bytes(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype, int32_t window_left)
{
    (void)causal;
    KvPlan pl;
    if (!plan_query(kKv8x256Words, bh_kv, 1, group, nq, nk, d, dtype, window_left, &pl)) return 0;
    return kv_workspace_bytes(pl, bh_kv, group, nq, d);
}

int32_t fa_kv8_256_splits_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype, int32_t window_left)
{
    (void)causal;
    KvPlan pl;
    if (!plan_query(kKv8x256Words, bh_kv, 1, group, nq, nk, d, dtype, window_left, &pl)) return 0;
    return pl.splits;
}

const char* fa_kv8_256_kernel_name_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype, int32_t window_left)
{
    (void)causal;
    KvPlan pl;
    if (!plan_query(kKv8x256Words, bh_kv, 1, group, nq, nk, d, dtype, window_left, &pl)) return nullptr;
    return kv8_256_decode_kernel_name();
}

int fa_kv8_256_forward(const void* q, const void* k8, const void* v8, void* o, float* lse, int64_t bh_kv, int32_t group, int64_t nq, int64_t nk,
                       int64_t capacity, const int32_t* kv_lens, int32_t d, float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype,
                       int32_t window_left, void* workspace, size_t workspace_bytes, void* stream)
{
    KvError& e = g_kv8_256_error;
    e.text[0] = 0;
    const KvCall a = {q, o, lse, bh_kv, 1, group, nq, nk, d, dtype, workspace, workspace_bytes};
    if (const int rc = check_cache(e, kKv8x256Words, a, k8, v8, capacity, kKv8x256Dims)) return rc;
    float folded;
    if (const int rc = check_scales(e, scale, k_scale, v_scale, &folded)) return rc;
    Kv8x256Params wp{};
    if (const int rc = check_window_or_none(e, window_left, &wp.window_left)) return rc;
    if (const int rc = plan_cache(e, kKv8x256Words, a, k8, v8, capacity, kv_lens, folded, wp.k8.pg.kv, span_or_none(nq, nk, wp.window_left))) return rc;
    return run(e, wp, d, v_scale, causal, a.out_f32(), 0, stream);
}

size_t fa_kv8_256_paged_workspace_bytes(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                                        int32_t window_left)
{
    (void)causal;
    KvPlan pl;
    if (!plan_query(kKv8x256PagedWords, batch, heads_kv, group, nq, nk, d, dtype, window_left, &pl)) return 0;
    return kv_workspace_bytes(pl, batch * heads_kv, group, nq, d);
}

int32_t fa_kv8_256_paged_splits_for(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                                    int32_t window_left)
{
    (void)causal;
    KvPlan pl;
    if (!plan_query(kKv8x256PagedWords, batch, heads_kv, group, nq, nk, d, dtype, window_left, &pl)) return 0;
    return pl.splits;
}

int fa_kv8_256_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse, int64_t batch, int32_t heads_kv, int32_t group, int64_t nq,
                             int64_t nk, int32_t d, float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype, int32_t window_left,
                             void* workspace, size_t workspace_bytes, void* stream)
{
    KvError& e = g_kv8_256_error;
    e.text[0] = 0;
    const KvCall a = {q, o, lse, batch, heads_kv, group, nq, nk, d, dtype, workspace, workspace_bytes};
    if (const int rc = check_pool(e, kKv8x256PagedWords, a, cache, kKv8x256Dims)) return rc;
    float folded;
    if (const int rc = check_scales(e, scale, k_scale, v_scale, &folded)) return rc;
    Kv8x256Params wp{};
    if (const int rc = check_window_or_none(e, window_left, &wp.window_left)) return rc;
    if (const int rc = plan_pool(e, kKv8x256PagedWords, a, *cache, folded, wp.k8.pg, span_or_none(nq, nk, wp.window_left))) return rc;
    return run(e, wp, d, v_scale, causal, a.out_f32(), 1, stream);
}

const char* fa_kv8_256_last_error(void) { return g_kv8_256_error.text; }

const char* fa_kv8_256_version(void)
{
    return "flashattn_amd_kv8_256 abi 1 gfx950 (K/V-cache attention at head dim 256 over an fp8 e4m3fn cache: contiguous and paged, optional sliding window)";
}

}  // extern "C"
