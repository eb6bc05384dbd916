// fa_kvpw256_prefill.hip -- the sliding-window chunked-prefill kernels of libflashattn_amd_kvpw.so at head dim 256 over a bf16 cache
// (contiguous or paged, causal or not, bf16 or fp32 output) and their launcher.  The loop is fa_kvp256_prefill_loop.h with WINDOW = true.
#include "fa_kvp256_prefill_loop.h"
#include "fa_kvpw.h"

namespace fa {

template <bool PAGED, bool CAUSAL, bool OUT_F32>
__global__ __launch_bounds__(kKvWaves* kWave) void fa_kvpw256_prefill_kernel(Kvpw256Params wp)
{
    kvp256_prefill<CAUSAL, OUT_F32, PAGED, true>(wp.p, wp.window_left);
}

using Kvpw256Kernel = void (*)(Kvpw256Params);

template <bool PAGED>
static Kvpw256Kernel pick(int causal, int out_f32)
{
    if (causal) return out_f32 ? fa_kvpw256_prefill_kernel<PAGED, true, true> : fa_kvpw256_prefill_kernel<PAGED, true, false>;
    return out_f32 ? fa_kvpw256_prefill_kernel<PAGED, false, true> : fa_kvpw256_prefill_kernel<PAGED, false, false>;
}

hipError_t launch_kvpw256_prefill(const Kvpw256Params& wp, int paged, int causal, int out_f32, hipStream_t stream)
{
    const KvParams& p = wp.p.pp.kv;
    if ((int64_t)p.bh_kv * wp.p.tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((int64_t)p.bh_kv * wp.p.tiles)), block(kKvWaves * kWave);
    hipLaunchKernelGGL(paged ? pick<true>(causal, out_f32) : pick<false>(causal, out_f32), grid, block, 0, stream, wp);
    return hipGetLastError();
}

}  // namespace fa
