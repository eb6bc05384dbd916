// fa_kv_combine.hip -- the merge kernel of libflashattn_amd_kv.so and, as the same object, of libflashattn_amd_paged.so: fa_kv_combine_kernel.h's
// body, unscaled.
#include "fa_kv_combine_kernel.h"

namespace fa {

template <bool OUT_F32>
__global__ __launch_bounds__(256) void fa_kv_combine_kernel(KvParams p, int d)
{
    kv_combine_body<OUT_F32, false>(p, d, 1.0f);
}

hipError_t launch_kv_combine(const KvParams& p, int d, int out_f32, hipStream_t stream)
{
    const unsigned blocks = kv_combine_blocks(p, d);
    if (blocks == 0) return hipErrorInvalidValue;
    if (out_f32)
        hipLaunchKernelGGL(fa_kv_combine_kernel<true>, dim3(blocks), dim3(256), 0, stream, p, d);
    else
        hipLaunchKernelGGL(fa_kv_combine_kernel<false>, dim3(blocks), dim3(256), 0, stream, p, d);
    return hipGetLastError();
}

}  // namespace fa
