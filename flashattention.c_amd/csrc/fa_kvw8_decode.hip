// fa_kvw8_decode.hip -- the decode kernel of libflashattn_amd_kvw8.so (sliding window over a contiguous and over a paged fp8 e4m3fn cache) and
// its launcher.  The loop is fa_kv8_decode_body.h with WINDOW = true: the same text the kernel of fa_kv8_decode.hip compiles.
#include "fa_kv8_decode_core.h"
#include "fa_kvw8.h"

namespace fa {

// d = 64: the unwindowed kernels fit 256 registers, two waves per SIMD; the window's row bound costs the contiguous ones four more unless the
// compiler is told that the second wave is wanted (no scratch either way: tests/test_kvw8_host.py).  d = 128 runs one wave per SIMD in both.
template <int D, bool CAUSAL, bool OUT_F32, bool PAGED>
__global__ __launch_bounds__(kKvWaves* kWave, D == 64 ? 2 : 1) void fa_kvw8_decode_kernel(Kvw8Params wp)
{
    constexpr bool WINDOW = true;
    const PagedParams& pp = wp.k8.pg;
    const KvParams& p = pp.kv;
    const float& v_scale = wp.k8.v_scale;
    const int window_left = wp.window_left;
#include "fa_kv8_decode_body.h"
}

template <int D, bool PAGED>
static hipError_t launch_decode_d(const Kvw8Params& wp, int causal, int out_f32, hipStream_t stream)
{
    const KvParams& p = wp.k8.pg.kv;
    const dim3 grid((unsigned)((int64_t)p.bh_kv * p.row_tiles * p.splits)), block(kKvWaves * kWave);
    if (causal) {
        if (out_f32)
            hipLaunchKernelGGL((fa_kvw8_decode_kernel<D, true, true, PAGED>), grid, block, 0, stream, wp);
        else
            hipLaunchKernelGGL((fa_kvw8_decode_kernel<D, true, false, PAGED>), grid, block, 0, stream, wp);
    } else {
        if (out_f32)
            hipLaunchKernelGGL((fa_kvw8_decode_kernel<D, false, true, PAGED>), grid, block, 0, stream, wp);
        else
            hipLaunchKernelGGL((fa_kvw8_decode_kernel<D, false, false, PAGED>), grid, block, 0, stream, wp);
    }
    return hipGetLastError();
}

hipError_t launch_kvw8_decode(const Kvw8Params& wp, int d, int causal, int out_f32, int paged, hipStream_t stream)
{
    const KvParams& p = wp.k8.pg.kv;
    if ((int64_t)p.bh_kv * p.row_tiles * p.splits > 0x7fffffffLL) return hipErrorInvalidValue;
    if (d == 64) return paged ? launch_decode_d<64, true>(wp, causal, out_f32, stream) : launch_decode_d<64, false>(wp, causal, out_f32, stream);
    if (d == 128) return paged ? launch_decode_d<128, true>(wp, causal, out_f32, stream) : launch_decode_d<128, false>(wp, causal, out_f32, stream);
    return hipErrorInvalidValue;
}

const char* kvw8_decode_kernel_name() { return "fa_kvw8_decode_kernel"; }

}  // namespace fa
