// fa_kvpw_prefill.hip -- the sliding-window chunked-prefill kernels of libflashattn_amd_kvpw.so at head dim 128 over a bf16 cache (contiguous
// or paged, causal or not, bf16 or fp32 output) and their launcher.  The loop is fa_kvp_prefill_loop.h with WINDOW = true.
#include "fa_kvp_prefill_loop.h"
#include "fa_kvpw.h"

namespace fa {

template <bool PAGED, bool CAUSAL, bool OUT_F32>
__global__ __launch_bounds__(kKvWaves* kWave) void fa_kvpw_prefill_kernel(KvpwParams wp)
{
    kvp_prefill<CAUSAL, OUT_F32, PAGED, false, KvpParams, true>(wp.p, wp.window_left);
}

using KvpwKernel = void (*)(KvpwParams);

template <bool PAGED>
static KvpwKernel pick(int causal, int out_f32)
{
    if (causal) return out_f32 ? fa_kvpw_prefill_kernel<PAGED, true, true> : fa_kvpw_prefill_kernel<PAGED, true, false>;
    return out_f32 ? fa_kvpw_prefill_kernel<PAGED, false, true> : fa_kvpw_prefill_kernel<PAGED, false, false>;
}

hipError_t launch_kvpw_prefill(const KvpwParams& wp, int paged, int causal, int out_f32, hipStream_t stream)
{
    const KvParams& p = wp.p.pp.kv;
    if ((int64_t)p.bh_kv * wp.p.tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((int64_t)p.bh_kv * wp.p.tiles)), block(kKvWaves * kWave);
    hipLaunchKernelGGL(paged ? pick<true>(causal, out_f32) : pick<false>(causal, out_f32), grid, block, 0, stream, wp);
    return hipGetLastError();
}

}  // namespace fa
