// fa_kvp256_prefill.hip -- the chunked-prefill kernels of libflashattn_amd_kvp256.so (head dim 256 over a bf16 cache: contiguous or paged,
// causal or not, bf16 or fp32 output) and their launcher.  The loop is fa_kvp256_prefill_loop.h.
#include "fa_kvp256_prefill_loop.h"

namespace fa {

template <bool PAGED, bool CAUSAL, bool OUT_F32>
__global__ __launch_bounds__(kKvWaves* kWave) void fa_kvp256_prefill_kernel(Kvp256Params wp)
{
    kvp256_prefill<CAUSAL, OUT_F32, PAGED>(wp);
}

using Kvp256Kernel = void (*)(Kvp256Params);

template <bool PAGED>
static Kvp256Kernel pick(int causal, int out_f32)
{
    if (causal) return out_f32 ? fa_kvp256_prefill_kernel<PAGED, true, true> : fa_kvp256_prefill_kernel<PAGED, true, false>;
    return out_f32 ? fa_kvp256_prefill_kernel<PAGED, false, true> : fa_kvp256_prefill_kernel<PAGED, false, false>;
}

hipError_t launch_kvp256_prefill(const Kvp256Params& wp, int paged, int causal, int out_f32, hipStream_t stream)
{
    const KvParams& p = wp.pp.kv;
    if ((int64_t)p.bh_kv * wp.tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((int64_t)p.bh_kv * wp.tiles)), block(kKvWaves * kWave);
    hipLaunchKernelGGL(paged ? pick<true>(causal, out_f32) : pick<false>(causal, out_f32), grid, block, 0, stream, wp);
    return hipGetLastError();
}

const char* kvp256_prefill_kernel_name() { return "fa_kvp256_prefill_kernel"; }

}  // namespace fa
