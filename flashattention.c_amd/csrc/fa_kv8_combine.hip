// fa_kv8_combine.hip -- the merge kernel of libflashattn_amd_kv8.so: fa_kv_combine_kernel.h's body with the multiplication by v_scale.
#include "fa_kv8.h"
#include "fa_kv_combine_kernel.h"

namespace fa {

template <bool OUT_F32>
__global__ __launch_bounds__(256) void fa_kv8_combine_kernel(KvParams p, int d, float v_scale)
{
    kv_combine_body<OUT_F32, true>(p, d, v_scale);
}

hipError_t launch_kv8_combine(const Kv8Params& p8, int d, int out_f32, hipStream_t stream)
{
    const KvParams& p = p8.pg.kv;
    const unsigned blocks = kv_combine_blocks(p, d);
    if (blocks == 0) return hipErrorInvalidValue;
    if (out_f32)
        hipLaunchKernelGGL(fa_kv8_combine_kernel<true>, dim3(blocks), dim3(256), 0, stream, p, d, p8.v_scale);
    else
        hipLaunchKernelGGL(fa_kv8_combine_kernel<false>, dim3(blocks), dim3(256), 0, stream, p, d, p8.v_scale);
    return hipGetLastError();
}

}  // namespace fa
