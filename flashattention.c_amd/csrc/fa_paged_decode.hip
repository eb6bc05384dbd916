// fa_paged_decode.hip -- the decode kernel of libflashattn_amd_paged.so (paged bf16 cache: the loop is fa_kv_decode16_body.h, which finds K/V
// rows through the block table) and its launcher.
#include "fa_kv_decode_core.h"

namespace fa {

template <int D, bool CAUSAL, bool OUT_F32>
__global__ __launch_bounds__(kKvWaves* kWave) void fa_paged_decode_kernel(PagedParams pp)
{
    constexpr bool PAGED = true, WINDOW = false;
    constexpr int P_TERMS = 2, window_left = 0;
    const KvParams& p = pp.kv;
#include "fa_kv_decode16_body.h"
}

template <int D>
static hipError_t launch_decode_d(const PagedParams& pp, int causal, int out_f32, hipStream_t stream)
{
    const KvParams& p = pp.kv;
    const dim3 grid((unsigned)((int64_t)p.bh_kv * p.row_tiles * p.splits)), block(kKvWaves * kWave);
    if (causal) {
        if (out_f32)
            hipLaunchKernelGGL((fa_paged_decode_kernel<D, true, true>), grid, block, 0, stream, pp);
        else
            hipLaunchKernelGGL((fa_paged_decode_kernel<D, true, false>), grid, block, 0, stream, pp);
    } else {
        if (out_f32)
            hipLaunchKernelGGL((fa_paged_decode_kernel<D, false, true>), grid, block, 0, stream, pp);
        else
            hipLaunchKernelGGL((fa_paged_decode_kernel<D, false, false>), grid, block, 0, stream, pp);
    }
    return hipGetLastError();
}

hipError_t launch_paged_decode(const PagedParams& pp, int d, int causal, int out_f32, hipStream_t stream)
{
    if ((int64_t)pp.kv.bh_kv * pp.kv.row_tiles * pp.kv.splits > 0x7fffffffLL) return hipErrorInvalidValue;
    if (d == 64) return launch_decode_d<64>(pp, causal, out_f32, stream);
    if (d == 128) return launch_decode_d<128>(pp, causal, out_f32, stream);
    return hipErrorInvalidValue;
}

const char* paged_decode_kernel_name() { return "fa_paged_decode_kernel"; }

}  // namespace fa
