// fa_kv_plan.cpp -- the entry points of include/flashattn_amd_kv.h over fa_kv_host.h (validation, plan, launch parameters).  The reference has
// no such operator; the conventions are those of include/flashattn_amd.h.
#include "fa_kv_host.h"
#include "flashattn_amd_kv.h"

namespace fa {

static thread_local KvError g_kv_error;
static const KvWords kKvWords = {2, "bh_kv", "caches are 16-bit", "bh_kv * group", "fa_kv_workspace_bytes", "k", "v", "q, k, v, o"};

}  // namespace fa

using namespace fa;

extern "C" {

size_t fa_kv_workspace_bytes(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype)
{
    (void)causal;
    if (check_shape(g_kv_error, kKvWords, bh_kv, 1, group, nq, nk, d, dtype) != FA_OK) return 0;
    return kv_workspace_bytes(kv_plan(bh_kv, group, nq, nk), bh_kv, group, nq, d);
}

int32_t fa_kv_splits_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype)
{
    (void)causal;
    if (check_shape(g_kv_error, kKvWords, bh_kv, 1, group, nq, nk, d, dtype) != FA_OK) return 0;
    return kv_plan(bh_kv, group, nq, nk).splits;
}

const char* fa_kv_kernel_name_for(int64_t bh_kv, int32_t group, int64_t nq, int64_t nk, int32_t d, int32_t causal, int32_t dtype)
{
    (void)causal;
    if (check_shape(g_kv_error, kKvWords, bh_kv, 1, group, nq, nk, d, dtype) != FA_OK) return nullptr;
    return kv_decode_kernel_name();
}

int fa_kv_forward(const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh_kv, int32_t group, int64_t nq, int64_t nk,
                  int64_t capacity, const int32_t* kv_lens, int32_t d, float scale, int32_t causal, int32_t dtype, void* workspace,
                  size_t workspace_bytes, void* stream)
{
    KvError& e = g_kv_error;
    e.text[0] = 0;
    const KvCall a = {q, o, lse, bh_kv, 1, group, nq, nk, d, dtype, workspace, workspace_bytes};
    if (const int rc = check_cache(e, kKvWords, a, k, v, capacity)) return rc;
    if (const int rc = check_scale(e, scale)) return rc;
    KvParams p{};
    if (const int rc = plan_cache(e, kKvWords, a, k, v, capacity, kv_lens, scale, p)) return rc;
    hipError_t err = launch_kv_decode(p, d, causal != 0, a.out_f32(), (hipStream_t)stream);
    if (err == hipSuccess && p.splits > 1) err = launch_kv_combine(p, d, a.out_f32(), (hipStream_t)stream);
    return launch_result(e, err);
}

int fa_kv_stream_read(const void* k, const void* v, int64_t bh_kv, int64_t nk, int64_t capacity, int32_t d, void* sink, void* stream)
{
    KvError& e = g_kv_error;
    e.text[0] = 0;
    if (k == nullptr || v == nullptr || sink == nullptr) return e.fail(FA_ERR_INVALID_ARGUMENT, "null pointer: k, v and sink are required");
    if (const int rc = check_shape(e, kKvWords, bh_kv, 1, 1, 1, nk, d, FA_DTYPE_BF16)) return rc;
    if (const int rc = check_capacity(e, kKvWords, nk, d, capacity)) return rc;
    if (((uintptr_t)k | (uintptr_t)v | (uintptr_t)sink) & 15) return e.fail(FA_ERR_INVALID_ARGUMENT, "k, v, sink must be 16-byte aligned");
    return launch_result(e, launch_kv_stream_read(k, v, bh_kv, nk, capacity, d, kv_plan(bh_kv, 1, 1, nk), (uint32_t*)sink, (hipStream_t)stream));
}

const char* fa_kv_last_error(void) { return g_kv_error.text; }

const char* fa_kv_version(void) { return "flashattn_amd_kv abi 1 gfx950 (K/V-cache attention: nq != nk, GQA, split-key decode)"; }

}  // extern "C"
