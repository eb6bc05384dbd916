// fa_kvp8_host.cpp -- the entry points of include/flashattn_amd_kvp8.h over fa_kv_host.h: those of fa_kvp_host.cpp (no workspace, d = 128 alone)
// over a cache of ONE byte per element with the two scales of fa_kv8_host.cpp (check_scales).
#include "fa_kv_host.h"
#include "fa_kvp8.h"
#include "flashattn_amd_kvp8.h"

namespace fa {

static thread_local KvError g_kvp8_error;
static const KvWords kKvp8Words = {1, "bh_kv", "q and o are as in fa_kv_forward", "bh_kv * group", "", "k8", "v8", "q, k8, v8, o"};
static const KvWords kKvp8PagedWords = {1, "batch, heads_kv", "q and o are as in fa_kv_forward", "batch * heads_kv * group", "", "k8", "v8", "q, k8, v8, o"};
static constexpr KvHeadDims kKvp8Dims = {kKvpHeadDim, kKvpHeadDim};

static int launch(Kvp8Params& wp, float v_scale, int paged, int causal, int out_f32, void* stream)
{
    wp.tiles = (wp.pp.kv.m_rows + kKvpRowTile - 1) / kKvpRowTile;
    wp.v_scale = v_scale;
    return launch_result(g_kvp8_error, launch_kvp8_prefill(wp, paged, causal, out_f32, (hipStream_t)stream));
}

}  // namespace fa

using namespace fa;

extern "C" {

const char* fa_kvp8_kernel_name_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype)
{
    (void)causal;
    if (check_shape(g_kvp8_error, kKvp8Words, bh_kv, 1, group, nq, nk, d, dtype, kKvp8Dims) != FA_OK) return nullptr;
    return kvp8_prefill_kernel_name();
}

int fa_kvp8_forward(const void* q, const void* k8, const void* v8, void* o, float* lse, int64_t bh_kv, int32_t group, int64_t nq, int64_t nk,
                    int64_t capacity, const int32_t* kv_lens, int32_t d, float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype,
                    void* stream)
{
    KvError& e = g_kvp8_error;
    e.text[0] = 0;
    const KvCall a = {q, o, lse, bh_kv, 1, group, nq, nk, d, dtype, nullptr, 0};
    if (const int rc = check_cache(e, kKvp8Words, a, k8, v8, capacity, kKvp8Dims)) return rc;
    float folded;
    if (const int rc = check_scales(e, scale, k_scale, v_scale, &folded)) return rc;
    Kvp8Params wp{};
    if (const int rc = plan_cache(e, kKvp8Words, a, k8, v8, capacity, kv_lens, folded, wp.pp.kv)) return rc;
    return launch(wp, v_scale, 0, causal != 0, a.out_f32(), stream);
}

int fa_kvp8_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse, int64_t batch, int32_t heads_kv, int32_t group, int64_t nq,
                          int64_t nk, int32_t d, float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype, void* stream)
{
    KvError& e = g_kvp8_error;
    e.text[0] = 0;
    const KvCall a = {q, o, lse, batch, heads_kv, group, nq, nk, d, dtype, nullptr, 0};
    if (const int rc = check_pool(e, kKvp8PagedWords, a, cache, kKvp8Dims)) return rc;
    float folded;
    if (const int rc = check_scales(e, scale, k_scale, v_scale, &folded)) return rc;
    Kvp8Params wp{};
    if (const int rc = plan_pool(e, kKvp8PagedWords, a, *cache, folded, wp.pp)) return rc;
    return launch(wp, v_scale, 1, causal != 0, a.out_f32(), stream);
}

const char* fa_kvp8_last_error(void) { return g_kvp8_error.text; }

const char* fa_kvp8_version(void)
{
    return "flashattn_amd_kvp8 abi 1 gfx950 (chunked prefill over fp8 e4m3fn K/V caches at head dim 128: contiguous and paged)";
}

}  // extern "C"
