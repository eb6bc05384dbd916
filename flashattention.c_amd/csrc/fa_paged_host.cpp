// fa_paged_host.cpp -- the entry points of include/flashattn_amd_paged.h over fa_kv_host.h (validation, plan, launch parameters).
#include "fa_kv_host.h"

namespace fa {

static thread_local KvError g_paged_error;
static const KvWords kPagedWords = {2, "batch, heads_kv", "caches are 16-bit", "batch * heads_kv * group", "fa_paged_workspace_bytes", "k", "v", "q, k, v, o"};

}  // namespace fa

using namespace fa;

extern "C" {

size_t fa_paged_workspace_bytes(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype)
{
    (void)causal;
    if (check_shape(g_paged_error, kPagedWords, batch, heads_kv, group, nq, nk, d, dtype) != FA_OK) return 0;
    return kv_workspace_bytes(kv_plan(batch * heads_kv, group, nq, nk), batch * heads_kv, group, nq, d);
}

int32_t fa_paged_splits_for(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype)
{
    (void)causal;
    if (check_shape(g_paged_error, kPagedWords, batch, heads_kv, group, nq, nk, d, dtype) != FA_OK) return 0;
    return kv_plan(batch * heads_kv, group, nq, nk).splits;
}

const char* fa_paged_kernel_name_for(int64_t batch, int32_t heads_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype,
                                     int32_t page_size)
{
    (void)causal;
    if (check_shape(g_paged_error, kPagedWords, batch, heads_kv, group, nq, nk, d, dtype) != FA_OK || check_page_size(g_paged_error, page_size) != FA_OK)
        return nullptr;
    return paged_decode_kernel_name();   // one family: the page size is a launch parameter
}

int fa_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse, int64_t batch, int32_t heads_kv, int32_t group, int64_t nq,
                     int64_t nk, int32_t d, float scale, int32_t causal, int32_t dtype, void* workspace, size_t workspace_bytes, void* stream)
{
    KvError& e = g_paged_error;
    e.text[0] = 0;
    const KvCall a = {q, o, lse, batch, heads_kv, group, nq, nk, d, dtype, workspace, workspace_bytes};
    if (const int rc = check_pool(e, kPagedWords, a, cache)) return rc;
    if (const int rc = check_scale(e, scale)) return rc;
    PagedParams pp{};
    if (const int rc = plan_pool(e, kPagedWords, a, *cache, scale, pp)) return rc;
    hipError_t err = launch_paged_decode(pp, d, causal != 0, a.out_f32(), (hipStream_t)stream);
    if (err == hipSuccess && pp.kv.splits > 1) err = launch_kv_combine(pp.kv, d, a.out_f32(), (hipStream_t)stream);
    return launch_result(e, err);
}

const char* fa_paged_last_error(void) { return g_paged_error.text; }

const char* fa_paged_version(void) { return "flashattn_amd_paged abi 1 gfx950 (paged K/V-cache attention: block tables over a shared page pool)"; }

}  // extern "C"
