// fa_kvpw_host.cpp -- the entry points of include/flashattn_amd_kvpw.h over fa_kv_host.h: those of fa_kvp_host.cpp, fa_kvp256_host.cpp (the bf16
// pair dispatches on d = 128 / 256) and fa_kvp8_host.cpp (the fp8 pair, d = 128) plus the window of fa_kvw_host.cpp (check_window: rejected
// below 0, saturated at 2^24).  No workspace and no key split, so the window never reaches the plan: it only travels to the kernel.
#include "fa_kv_host.h"
#include "fa_kvpw.h"
#include "flashattn_amd_kvpw.h"

namespace fa {

static thread_local KvError g_kvpw_error;
static const KvWords kKvpwWords = {2, "bh_kv", "caches are 16-bit", "bh_kv * group", "", "k", "v", "q, k, v, o"};
static const KvWords kKvpwPagedWords = {2, "batch, heads_kv", "caches are 16-bit", "batch * heads_kv * group", "", "k", "v", "q, k, v, o"};
static const KvWords kKvpw8Words = {1, "bh_kv", "q and o are as in fa_kv_forward", "bh_kv * group", "", "k8", "v8", "q, k8, v8, o"};
static const KvWords kKvpw8PagedWords = {1, "batch, heads_kv", "q and o are as in fa_kv_forward", "batch * heads_kv * group", "", "k8", "v8", "q, k8, v8, o"};
static constexpr KvHeadDims kKvpwDims = {kKvpHeadDim, kKvp256HeadDim};
static constexpr KvHeadDims kKvpw8Dims = {kKvpHeadDim, kKvpHeadDim};

// the bf16 launch at either head dim: pp is filled (plan_cache / plan_pool), the tiles are those of the head dim's kernel
static int launch(const PagedParams& pp, int32_t d, int32_t window_left, int paged, int causal, int out_f32, void* stream)
{
    if (d == kKvp256HeadDim) {
        const Kvpw256Params wp = {{pp, (pp.kv.m_rows + kKvp256RowTile - 1) / kKvp256RowTile}, window_left};
        return launch_result(g_kvpw_error, launch_kvpw256_prefill(wp, paged, causal, out_f32, (hipStream_t)stream));
    }
    const KvpwParams wp = {{pp, (pp.kv.m_rows + kKvpRowTile - 1) / kKvpRowTile}, window_left};
    return launch_result(g_kvpw_error, launch_kvpw_prefill(wp, paged, causal, out_f32, (hipStream_t)stream));
}

static int launch8(const PagedParams& pp, float v_scale, int32_t window_left, int paged, int causal, int out_f32, void* stream)
{
    const Kvpw8Params wp = {{pp, (pp.kv.m_rows + kKvpRowTile - 1) / kKvpRowTile, v_scale}, window_left};
    return launch_result(g_kvpw_error, launch_kvpw8_prefill(wp, paged, causal, out_f32, (hipStream_t)stream));
}

}  // namespace fa

using namespace fa;

extern "C" {

const char* fa_kvpw_kernel_name_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype, int32_t window_left)
{
    (void)causal;
    int32_t w;
    if (check_shape(g_kvpw_error, kKvpwWords, bh_kv, 1, group, nq, nk, d, dtype, kKvpwDims) != FA_OK || check_window(g_kvpw_error, window_left, &w) != FA_OK)
        return nullptr;
    return d == kKvp256HeadDim ? "fa_kvpw256_prefill_kernel" : "fa_kvpw_prefill_kernel";
}

int fa_kvpw_forward(const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh_kv, int32_t group, int64_t nq, int64_t nk,
                    int64_t capacity, const int32_t* kv_lens, int32_t d, float scale, int32_t causal, int32_t dtype, int32_t window_left, void* stream)
{
    KvError& e = g_kvpw_error;
    e.text[0] = 0;
    const KvCall a = {q, o, lse, bh_kv, 1, group, nq, nk, d, dtype, nullptr, 0};
    if (const int rc = check_cache(e, kKvpwWords, a, k, v, capacity, kKvpwDims)) return rc;
    if (const int rc = check_scale(e, scale)) return rc;
    int32_t w;
    if (const int rc = check_window(e, window_left, &w)) return rc;
    PagedParams pp{};
    if (const int rc = plan_cache(e, kKvpwWords, a, k, v, capacity, kv_lens, scale, pp.kv)) return rc;
    return launch(pp, d, w, 0, causal != 0, a.out_f32(), stream);
}

int fa_kvpw_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse, int64_t batch, int32_t heads_kv, int32_t group, int64_t nq,
                          int64_t nk, int32_t d, float scale, int32_t causal, int32_t dtype, int32_t window_left, void* stream)
{
    KvError& e = g_kvpw_error;
    e.text[0] = 0;
    const KvCall a = {q, o, lse, batch, heads_kv, group, nq, nk, d, dtype, nullptr, 0};
    if (const int rc = check_pool(e, kKvpwPagedWords, a, cache, kKvpwDims)) return rc;
    if (const int rc = check_scale(e, scale)) return rc;
    int32_t w;
    if (const int rc = check_window(e, window_left, &w)) return rc;
    PagedParams pp{};
    if (const int rc = plan_pool(e, kKvpwPagedWords, a, *cache, scale, pp)) return rc;
    return launch(pp, d, w, 1, causal != 0, a.out_f32(), stream);
}

int fa_kvpw_fp8_forward(const void* q, const void* k8, const void* v8, void* o, float* lse, int64_t bh_kv, int32_t group, int64_t nq, int64_t nk,
                        int64_t capacity, const int32_t* kv_lens, int32_t d, float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype,
                        int32_t window_left, void* stream)
{
    KvError& e = g_kvpw_error;
    e.text[0] = 0;
    const KvCall a = {q, o, lse, bh_kv, 1, group, nq, nk, d, dtype, nullptr, 0};
    if (const int rc = check_cache(e, kKvpw8Words, a, k8, v8, capacity, kKvpw8Dims)) return rc;
    float folded;
    if (const int rc = check_scales(e, scale, k_scale, v_scale, &folded)) return rc;
    int32_t w;
    if (const int rc = check_window(e, window_left, &w)) return rc;
    PagedParams pp{};
    if (const int rc = plan_cache(e, kKvpw8Words, a, k8, v8, capacity, kv_lens, folded, pp.kv)) return rc;
    return launch8(pp, v_scale, w, 0, causal != 0, a.out_f32(), stream);
}

int fa_kvpw_fp8_paged_forward(const void* q, const fa_paged_cache* cache, void* o, float* lse, int64_t batch, int32_t heads_kv, int32_t group,
                              int64_t nq, int64_t nk, int32_t d, float scale, float k_scale, float v_scale, int32_t causal, int32_t dtype,
                              int32_t window_left, void* stream)
{
    KvError& e = g_kvpw_error;
    e.text[0] = 0;
    const KvCall a = {q, o, lse, batch, heads_kv, group, nq, nk, d, dtype, nullptr, 0};
    if (const int rc = check_pool(e, kKvpw8PagedWords, a, cache, kKvpw8Dims)) return rc;
    float folded;
    if (const int rc = check_scales(e, scale, k_scale, v_scale, &folded)) return rc;
    int32_t w;
    if (const int rc = check_window(e, window_left, &w)) return rc;
    PagedParams pp{};
    if (const int rc = plan_pool(e, kKvpw8PagedWords, a, *cache, folded, pp)) return rc;
    return launch8(pp, v_scale, w, 1, causal != 0, a.out_f32(), stream);
}

const char* fa_kvpw_last_error(void) { return g_kvpw_error.text; }

const char* fa_kvpw_version(void)
{
    return "flashattn_amd_kvpw abi 1 gfx950 (sliding-window chunked prefill over K/V caches: bf16 at head dims 128 and 256, fp8 e4m3fn at 128; contiguous and paged)";
}

}  // extern "C"
