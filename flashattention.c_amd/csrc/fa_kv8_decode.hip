// fa_kv8_decode.hip -- the decode kernel of libflashattn_amd_kv8.so: fa_kv_decode_core.h's workgroup, arithmetic, merge and page walk over a
// cache of 8-bit floats (OCP e4m3fn, one byte per element), contiguous or paged, with a loop of its own: fa_kv8_decode_body.h with
// WINDOW = false, the same text the kernel of fa_kvw8_decode.hip compiles with WINDOW = true.  No counterpart in the reference.
#include "fa_kv8.h"
#include "fa_kv8_decode_core.h"

namespace fa {

template <int D, bool CAUSAL, bool OUT_F32, bool PAGED>
__global__ __launch_bounds__(kKvWaves* kWave) void fa_kv8_decode_kernel(Kv8Params p8)
{
    constexpr bool WINDOW = false;
    constexpr int window_left = 0;   // never read
    const PagedParams& pp = p8.pg;
    const KvParams& p = pp.kv;
    const float& v_scale = p8.v_scale;
#include "fa_kv8_decode_body.h"
}

template <int D, bool PAGED>
static hipError_t launch_decode_d(const Kv8Params& p8, int causal, int out_f32, hipStream_t stream)
{
    const KvParams& p = p8.pg.kv;
    const dim3 grid((unsigned)((int64_t)p.bh_kv * p.row_tiles * p.splits)), block(kKvWaves * kWave);
    if (causal) {
        if (out_f32)
            hipLaunchKernelGGL((fa_kv8_decode_kernel<D, true, true, PAGED>), grid, block, 0, stream, p8);
        else
            hipLaunchKernelGGL((fa_kv8_decode_kernel<D, true, false, PAGED>), grid, block, 0, stream, p8);
    } else {
        if (out_f32)
            hipLaunchKernelGGL((fa_kv8_decode_kernel<D, false, true, PAGED>), grid, block, 0, stream, p8);
        else
            hipLaunchKernelGGL((fa_kv8_decode_kernel<D, false, false, PAGED>), grid, block, 0, stream, p8);
    }
    return hipGetLastError();
}

hipError_t launch_kv8_decode(const Kv8Params& p8, int d, int causal, int out_f32, int paged, hipStream_t stream)
{
    const KvParams& p = p8.pg.kv;
    if ((int64_t)p.bh_kv * p.row_tiles * p.splits > 0x7fffffffLL) return hipErrorInvalidValue;
    if (d == 64) return paged ? launch_decode_d<64, true>(p8, causal, out_f32, stream) : launch_decode_d<64, false>(p8, causal, out_f32, stream);
    if (d == 128) return paged ? launch_decode_d<128, true>(p8, causal, out_f32, stream) : launch_decode_d<128, false>(p8, causal, out_f32, stream);
    return hipErrorInvalidValue;
}

const char* kv8_decode_kernel_name() { return "fa_kv8_decode_kernel"; }

}  // namespace fa
