// fa_kv8_256_decode.hip -- the decode kernels of libflashattn_amd_kv8_256.so (head dim 256 over an fp8 e4m3fn cache: contiguous or paged, with or
// without a sliding window, causal or not, bf16 or fp32 output) and their launcher.  The loop is fa_kv8_256_decode_loop.h.
#include "fa_kv8_256_decode_loop.h"

namespace fa {

template <bool PAGED, bool WINDOW, bool CAUSAL, bool OUT_F32>
__global__ __launch_bounds__(kKvWaves* kWave) void fa_kv8_256_decode_kernel(Kv8x256Params wp)
{
    kv8_256_decode<CAUSAL, OUT_F32, PAGED, WINDOW>(wp);
}

using Kv8x256Kernel = void (*)(Kv8x256Params);

template <bool PAGED, bool WINDOW>
static Kv8x256Kernel pick(int causal, int out_f32)
{
    if (causal) return out_f32 ? fa_kv8_256_decode_kernel<PAGED, WINDOW, true, true> : fa_kv8_256_decode_kernel<PAGED, WINDOW, true, false>;
    return out_f32 ? fa_kv8_256_decode_kernel<PAGED, WINDOW, false, true> : fa_kv8_256_decode_kernel<PAGED, WINDOW, false, false>;
}

hipError_t launch_kv8_256_decode(const Kv8x256Params& wp, int paged, int window, int causal, int out_f32, hipStream_t stream)
{
    const KvParams& p = wp.k8.pg.kv;
    if ((int64_t)p.bh_kv * p.row_tiles * p.splits > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((int64_t)p.bh_kv * p.row_tiles * p.splits)), block(kKvWaves * kWave);
    const Kv8x256Kernel kernel = paged ? (window ? pick<true, true>(causal, out_f32) : pick<true, false>(causal, out_f32))
                                       : (window ? pick<false, true>(causal, out_f32) : pick<false, false>(causal, out_f32));
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, wp);
    return hipGetLastError();
}

const char* kv8_256_decode_kernel_name() { return "fa_kv8_256_decode_kernel"; }

}  // namespace fa
