// fa_kvpw8_prefill.hip -- the sliding-window chunked-prefill kernels of libflashattn_amd_kvpw.so at head dim 128 over an fp8 e4m3fn cache
// (contiguous or paged, causal or not, bf16 or fp32 output) and their launcher.  The loop is fa_kvp_prefill_loop.h with FP8 and WINDOW = true.
#include "fa_kvp_prefill_loop.h"
#include "fa_kvpw.h"

namespace fa {

template <bool PAGED, bool CAUSAL, bool OUT_F32>
__global__ __launch_bounds__(kKvWaves* kWave) void fa_kvpw8_prefill_kernel(Kvpw8Params wp)
{
    kvp_prefill<CAUSAL, OUT_F32, PAGED, true, Kvp8Params, true>(wp.p, wp.window_left);
}

using Kvpw8Kernel = void (*)(Kvpw8Params);

template <bool PAGED>
static Kvpw8Kernel pick(int causal, int out_f32)
{
    if (causal) return out_f32 ? fa_kvpw8_prefill_kernel<PAGED, true, true> : fa_kvpw8_prefill_kernel<PAGED, true, false>;
    return out_f32 ? fa_kvpw8_prefill_kernel<PAGED, false, true> : fa_kvpw8_prefill_kernel<PAGED, false, false>;
}

hipError_t launch_kvpw8_prefill(const Kvpw8Params& wp, int paged, int causal, int out_f32, hipStream_t stream)
{
    const KvParams& p = wp.p.pp.kv;
    if ((int64_t)p.bh_kv * wp.p.tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((int64_t)p.bh_kv * wp.p.tiles)), block(kKvWaves * kWave);
    hipLaunchKernelGGL(paged ? pick<true>(causal, out_f32) : pick<false>(causal, out_f32), grid, block, 0, stream, wp);
    return hipGetLastError();
}

}  // namespace fa
