// fa_kv8_host.cpp -- the entry points of include/flashattn_amd_kv8.h over fa_kv_host.h (validation, plan, launch parameters) with an element of
// ONE byte and the two scales of the cache (check_scales).
#include "fa_kv8.h"
#include "fa_kv_host.h"
#include "flashattn_amd_kv8.h"

namespace fa {

static thread_local KvError g_kv8_error;
static const KvWords kKv8Words = {1, "bh_kv (batch, heads_kv)", "q and o are as in fa_kv_forward", "bh_kv * group (batch * heads_kv * group)", "fa_kv8_workspace_bytes",
                                  "k8", "v8", "q, k8, v8, o"};

static int run(KvError& e, Kv8Params& p8, int32_t d, float v_scale, int32_t causal, int out_f32, int paged, void* stream)
{
    p8.v_scale = v_scale;
    hipError_t err = launch_kv8_decode(p8, d, causal != 0, out_f32, paged, (hipStream_t)stream);
    if (err == hipSuccess && p8.pg.kv.splits > 1) err = launch_kv8_combine(p8, d, out_f32, (hipStream_t)stream);
    return launch_result(e, err);
}

}  // namespace fa

using namespace fa;

extern "C" {

size_t fa_kv8_workspace_bytes(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype)
{
    (void)causal;
    if (check_shape(g_kv8_error, kKv8Words, bh_kv, 1, group, nq, nk, d, dtype) != FA_OK) return 0;
    return kv_workspace_bytes(kv_plan(bh_kv, group, nq, nk), bh_kv, group, nq, d);
}

int32_t fa_kv8_splits_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype)
{
    (void)causal;
    if (check_shape(g_kv8_error, kKv8Words, bh_kv, 1, group, nq, nk, d, dtype) != FA_OK) return 0;
    return kv_plan(bh_kv, group, nq, nk).splits;
}

const char* fa_kv8_kernel_name_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype, int32_t page_size)
{
    (void)causal;
    if (check_shape(g_kv8_error, kKv8Words, bh_kv, 1, group, nq, nk, d, dtype) != FA_OK) return nullptr;
    if (page_size != 0 && check_page_size(g_kv8_error, page_size) != FA_OK) return nullptr;
    return kv8_decode_kernel_name();   // one family: paged or not is a template argument, the page size a launch parameter
}

int fa_kv8_forward(const void* q, const void* k8, const void* v8, void* o, float* lse, int64_t bh_kv, int32_t group, int64_t nq, int64_t nk,
                   int64_t capacity, const int32_t* kv_lens, int32_t d, float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype,
                   void* workspace, size_t workspace_bytes, void* stream)
{
    KvError& e = g_kv8_error;
    e.text[0] = 0;
    const KvCall a = {q, o, lse, bh_kv, 1, group, nq, nk, d, dtype, workspace, workspace_bytes};
    if (const int rc = check_cache(e, kKv8Words, a, k8, v8, capacity)) return rc;
    float folded;
    if (const int rc = check_scales(e, scale, k_scale, v_scale, &folded)) return rc;
    Kv8Params p8{};
    if (const int rc = plan_cache(e, kKv8Words, a, k8, v8, capacity, kv_lens, folded, p8.pg.kv)) return rc;
    return run(e, p8, d, v_scale, causal, a.out_f32(), 0, stream);
}

int fa_kv8_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse, int64_t batch, int32_t heads_kv, int32_t group, int64_t nq,
                         int64_t nk, int32_t d, float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype, void* workspace,
                         size_t workspace_bytes, void* stream)
{
    KvError& e = g_kv8_error;
    e.text[0] = 0;
    const KvCall a = {q, o, lse, batch, heads_kv, group, nq, nk, d, dtype, workspace, workspace_bytes};
    if (const int rc = check_pool(e, kKv8Words, a, cache)) return rc;
    float folded;
    if (const int rc = check_scales(e, scale, k_scale, v_scale, &folded)) return rc;
    Kv8Params p8{};
    if (const int rc = plan_pool(e, kKv8Words, a, *cache, folded, p8.pg)) return rc;
    return run(e, p8, d, v_scale, causal, a.out_f32(), 1, stream);
}

const char* fa_kv8_last_error(void) { return g_kv8_error.text; }

const char* fa_kv8_version(void) { return "flashattn_amd_kv8 abi 1 gfx950 (K/V-cache attention over an fp8 e4m3fn cache, contiguous and paged)"; }

}  // extern "C"
