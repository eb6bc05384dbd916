// fa_kvp256_host.cpp -- the entry points of include/flashattn_amd_kvp256.h over fa_kv_host.h: its validation and its fill of the launch
// parameters, with no workspace (the calls are always "unsplit" to the validators: the prefill kernel has no key split), at d = 256 alone.
#include "fa_kv_host.h"
#include "fa_kvp256.h"
#include "flashattn_amd_kvp256.h"

namespace fa {

static thread_local KvError g_kvp256_error;
static const KvWords kKvp256Words = {2, "bh_kv", "caches are 16-bit", "bh_kv * group", "", "k", "v", "q, k, v, o"};
static const KvWords kKvp256PagedWords = {2, "batch, heads_kv", "caches are 16-bit", "batch * heads_kv * group", "", "k", "v", "q, k, v, o"};
static constexpr KvHeadDims kKvp256Dims = {kKvp256HeadDim, kKvp256HeadDim};

static int launch(Kvp256Params& wp, int paged, int causal, int out_f32, void* stream)
{
    wp.tiles = (wp.pp.kv.m_rows + kKvp256RowTile - 1) / kKvp256RowTile;
    return launch_result(g_kvp256_error, launch_kvp256_prefill(wp, paged, causal, out_f32, (hipStream_t)stream));
}

}  // namespace fa

using namespace fa;

extern "C" {

const char* fa_kvp256_kernel_name_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype)
{
    (void)causal;
    if (check_shape(g_kvp256_error, kKvp256Words, bh_kv, 1, group, nq, nk, d, dtype, kKvp256Dims) != FA_OK) return nullptr;
    return kvp256_prefill_kernel_name();
}

int fa_kvp256_forward(const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh_kv, int32_t group, int64_t nq, int64_t nk,
                      int64_t capacity, const int32_t* kv_lens, int32_t d, float scale, int32_t causal, int32_t dtype, void* stream)
{
    KvError& e = g_kvp256_error;
    e.text[0] = 0;
    const KvCall a = {q, o, lse, bh_kv, 1, group, nq, nk, d, dtype, nullptr, 0};
    if (const int rc = check_cache(e, kKvp256Words, a, k, v, capacity, kKvp256Dims)) return rc;
    if (const int rc = check_scale(e, scale)) return rc;
    Kvp256Params wp{};
    if (const int rc = plan_cache(e, kKvp256Words, a, k, v, capacity, kv_lens, scale, wp.pp.kv)) return rc;
    return launch(wp, 0, causal != 0, a.out_f32(), stream);
}

int fa_kvp256_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse, int64_t batch, int32_t heads_kv, int32_t group,
                            int64_t nq, int64_t nk, int32_t d, float scale, int32_t causal, int32_t dtype, void* stream)
{
    KvError& e = g_kvp256_error;
    e.text[0] = 0;
    const KvCall a = {q, o, lse, batch, heads_kv, group, nq, nk, d, dtype, nullptr, 0};
    if (const int rc = check_pool(e, kKvp256PagedWords, a, cache, kKvp256Dims)) return rc;
    if (const int rc = check_scale(e, scale)) return rc;
    Kvp256Params wp{};
    if (const int rc = plan_pool(e, kKvp256PagedWords, a, *cache, scale, wp.pp)) return rc;
    return launch(wp, 1, causal != 0, a.out_f32(), stream);
}

const char* fa_kvp256_last_error(void) { return g_kvp256_error.text; }

const char* fa_kvp256_version(void) { return "flashattn_amd_kvp256 abi 1 gfx950 (chunked prefill over bf16 K/V caches at head dim 256: contiguous and paged)"; }

}  // extern "C"
