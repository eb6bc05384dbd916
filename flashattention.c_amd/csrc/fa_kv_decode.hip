// fa_kv_decode.hip -- the decode kernel of libflashattn_amd_kv.so (contiguous bf16 cache: the loop is fa_kv_decode16_body.h), its launcher, and
// the stream-read kernel that measures the bandwidth floor.
#include "fa_kv_decode_core.h"

namespace fa {

#ifndef FA_KV_P_TERMS
#define FA_KV_P_TERMS 2   // 1: measurement builds only (profiles/kv_decode.py: is the second P.V product free?)
#endif

template <int D, bool CAUSAL, bool OUT_F32>
__global__ __launch_bounds__(kKvWaves* kWave) void fa_kv_decode_kernel(KvParams p)
{
    constexpr bool PAGED = false, WINDOW = false;
    constexpr int P_TERMS = FA_KV_P_TERMS, window_left = 0;
    constexpr PagedParams pp{};   // never read
#include "fa_kv_decode16_body.h"
}

// ---- the bandwidth floor: the same K/V bytes (rows [0, nk) of every slab), the same share per workgroup, 16-byte loads, XOR-folded ----
__global__ __launch_bounds__(kKvWaves* kWave) void fa_kv_stream_read_kernel(const u32x4* __restrict__ k, const u32x4* __restrict__ v, int64_t slab_vecs,
                                                                             int row_vecs, int nk, int splits, int share, uint32_t* __restrict__ sink)
{
    __shared__ uint32_t red[kKvWaves * kWave];
    const int s_idx = blockIdx.x % splits, slab = blockIdx.x / splits;
    const int kbeg = s_idx * share, kend = min(kbeg + share, nk);
    const int64_t base = slab * slab_vecs + (int64_t)kbeg * row_vecs;
    const int nvec = max(kend - kbeg, 0) * row_vecs;
    u32x4 acc = {0u, 0u, 0u, 0u};
#pragma unroll 8
    for (int i = threadIdx.x; i < nvec; i += kKvWaves * kWave) acc ^= k[base + i] ^ v[base + i];
    red[threadIdx.x] = acc[0] ^ acc[1] ^ acc[2] ^ acc[3];
    __syncthreads();
    for (int w = kKvWaves * kWave / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] ^= red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) sink[blockIdx.x % 1024] = red[0];
}

template <int D>
static hipError_t launch_decode_d(const KvParams& p, int causal, int out_f32, hipStream_t stream)
{
    const dim3 grid((unsigned)((int64_t)p.bh_kv * p.row_tiles * p.splits)), block(kKvWaves * kWave);
    if (causal) {
        if (out_f32)
            hipLaunchKernelGGL((fa_kv_decode_kernel<D, true, true>), grid, block, 0, stream, p);
        else
            hipLaunchKernelGGL((fa_kv_decode_kernel<D, true, false>), grid, block, 0, stream, p);
    } else {
        if (out_f32)
            hipLaunchKernelGGL((fa_kv_decode_kernel<D, false, true>), grid, block, 0, stream, p);
        else
            hipLaunchKernelGGL((fa_kv_decode_kernel<D, false, false>), grid, block, 0, stream, p);
    }
    return hipGetLastError();
}

hipError_t launch_kv_decode(const KvParams& p, int d, int causal, int out_f32, hipStream_t stream)
{
    if ((int64_t)p.bh_kv * p.row_tiles * p.splits > 0x7fffffffLL) return hipErrorInvalidValue;
    if (d == 64) return launch_decode_d<64>(p, causal, out_f32, stream);
    if (d == 128) return launch_decode_d<128>(p, causal, out_f32, stream);
    return hipErrorInvalidValue;
}

hipError_t launch_kv_stream_read(const void* k, const void* v, int64_t bh_kv, int64_t nk, int64_t capacity, int d, const KvPlan& pl, uint32_t* sink,
                                 hipStream_t stream)
{
    if (bh_kv * pl.splits > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fa_kv_stream_read_kernel, dim3((unsigned)(bh_kv * pl.splits)), dim3(kKvWaves * kWave), 0, stream, (const u32x4*)k, (const u32x4*)v,
                       capacity * d / 8, d / 8, (int)nk, pl.splits, pl.share, sink);
    return hipGetLastError();
}

const char* kv_decode_kernel_name() { return "fa_kv_decode_kernel"; }

}  // namespace fa
