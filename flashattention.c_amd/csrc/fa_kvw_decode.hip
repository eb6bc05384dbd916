// fa_kvw_decode.hip -- the two decode kernels of libflashattn_amd_kvw.so (sliding window over a contiguous and over a paged bf16 cache) and their
// launchers.  The loop is fa_kv_decode16_body.h with WINDOW = true: the same text the kernels of fa_kv_decode.hip and fa_paged_decode.hip compile.
#include "fa_kv_decode_core.h"
#include "fa_kvw.h"

namespace fa {

template <int D, bool CAUSAL, bool OUT_F32>
__global__ __launch_bounds__(kKvWaves* kWave) void fa_kvw_decode_kernel(KvwParams wp)
{
    constexpr bool PAGED = false, WINDOW = true;
    constexpr int P_TERMS = 2;
    constexpr PagedParams pp{};   // never read
    const KvParams& p = wp.kv;
    const int window_left = wp.window_left;
#include "fa_kv_decode16_body.h"
}

template <int D, bool CAUSAL, bool OUT_F32>
__global__ __launch_bounds__(kKvWaves* kWave) void fa_kvw_paged_decode_kernel(KvwPagedParams wp)
{
    constexpr bool PAGED = true, WINDOW = true;
    constexpr int P_TERMS = 2;
    const PagedParams& pp = wp.pp;
    const KvParams& p = pp.kv;
    const int window_left = wp.window_left;
#include "fa_kv_decode16_body.h"
}

template <int D>
static hipError_t launch_decode_d(const KvwParams& wp, int causal, int out_f32, hipStream_t stream)
{
    const KvParams& p = wp.kv;
    const dim3 grid((unsigned)((int64_t)p.bh_kv * p.row_tiles * p.splits)), block(kKvWaves * kWave);
    if (causal) {
        if (out_f32)
            hipLaunchKernelGGL((fa_kvw_decode_kernel<D, true, true>), grid, block, 0, stream, wp);
        else
            hipLaunchKernelGGL((fa_kvw_decode_kernel<D, true, false>), grid, block, 0, stream, wp);
    } else {
        if (out_f32)
            hipLaunchKernelGGL((fa_kvw_decode_kernel<D, false, true>), grid, block, 0, stream, wp);
        else
            hipLaunchKernelGGL((fa_kvw_decode_kernel<D, false, false>), grid, block, 0, stream, wp);
    }
    return hipGetLastError();
}

template <int D>
static hipError_t launch_paged_decode_d(const KvwPagedParams& wp, int causal, int out_f32, hipStream_t stream)
{
    const KvParams& p = wp.pp.kv;
    const dim3 grid((unsigned)((int64_t)p.bh_kv * p.row_tiles * p.splits)), block(kKvWaves * kWave);
    if (causal) {
        if (out_f32)
            hipLaunchKernelGGL((fa_kvw_paged_decode_kernel<D, true, true>), grid, block, 0, stream, wp);
        else
            hipLaunchKernelGGL((fa_kvw_paged_decode_kernel<D, true, false>), grid, block, 0, stream, wp);
    } else {
        if (out_f32)
            hipLaunchKernelGGL((fa_kvw_paged_decode_kernel<D, false, true>), grid, block, 0, stream, wp);
        else
            hipLaunchKernelGGL((fa_kvw_paged_decode_kernel<D, false, false>), grid, block, 0, stream, wp);
    }
    return hipGetLastError();
}

hipError_t launch_kvw_decode(const KvwParams& wp, int d, int causal, int out_f32, hipStream_t stream)
{
    if ((int64_t)wp.kv.bh_kv * wp.kv.row_tiles * wp.kv.splits > 0x7fffffffLL) return hipErrorInvalidValue;
    if (d == 64) return launch_decode_d<64>(wp, causal, out_f32, stream);
    if (d == 128) return launch_decode_d<128>(wp, causal, out_f32, stream);
    return hipErrorInvalidValue;
}

hipError_t launch_kvw_paged_decode(const KvwPagedParams& wp, int d, int causal, int out_f32, hipStream_t stream)
{
    if ((int64_t)wp.pp.kv.bh_kv * wp.pp.kv.row_tiles * wp.pp.kv.splits > 0x7fffffffLL) return hipErrorInvalidValue;
    if (d == 64) return launch_paged_decode_d<64>(wp, causal, out_f32, stream);
    if (d == 128) return launch_paged_decode_d<128>(wp, causal, out_f32, stream);
    return hipErrorInvalidValue;
}

const char* kvw_decode_kernel_name() { return "fa_kvw_decode_kernel"; }
const char* kvw_paged_decode_kernel_name() { return "fa_kvw_paged_decode_kernel"; }

}  // namespace fa
