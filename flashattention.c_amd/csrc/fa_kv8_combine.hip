// fa_kv8_combine.hip -- the merge of a key-split forward over an fp8 cache: fa_kv_combine.hip (that file explains the method) with ONE more
// operation, the multiplication of the merged, normalised row by v_scale in front of the store.
//
// Why the library does not link fa_kv_combine.hip's object as the paged one does: that kernel has nowhere to take v_scale from, so the key
// shares would have to store partial outputs that are scaled already.  The merge forms sum_s w_s O_s / sum_s w_s with one fused multiply-add
// per share in the numerator and the same sequence against 1 in the denominator; the quotient of the two is exact where every O_s is 1 (a
// constant V), and off by a few ulp where every O_s is fp32(0.37) -- measured: 512 of 1024 elements, up to 3 ulp, at 1 x 8 x 1 x 8192 x 128.
// With the scale applied here, behind the quotient, a constant V comes out as fp32(v_scale * constant) from split launches as it does from
// unsplit ones, and everything in front of it is the bf16 merge instruction for instruction: with v_scale a power of two the result is still
// v_scale x the bf16 library's, bit for bit.
#include "fa_kv8.h"

namespace fa {

constexpr int kKv8CombineBatch = 16;

template <bool OUT_F32>
__global__ __launch_bounds__(256) void fa_kv8_combine_kernel(KvParams p, int d, float v_scale)
{
    const int tpr = d / 4;
    const int64_t rows = (int64_t)p.bh_kv * p.m_rows;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t row = t / tpr;
    if (row >= rows) return;
    const int c = (int)(t % tpr) * 4;
    const int S = p.splits;

    float l[kKvMaxSplits];
#pragma unroll
    for (int s = 0; s < kKvMaxSplits; ++s) l[s] = s < S ? p.lse_part[(int64_t)s * rows + row] : -INFINITY;
    float m = l[0];
#pragma unroll
    for (int s = 1; s < kKvMaxSplits; ++s) m = fmaxf(m, l[s]);
    const bool none = m == -INFINITY;

    float wsum = 0.0f;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s0 = 0; s0 < kKvMaxSplits; s0 += kKv8CombineBatch) {
        if (s0 >= S) break;   // uniform
        f32x4 x[kKv8CombineBatch];
#pragma unroll
        for (int i = 0; i < kKv8CombineBatch; ++i)
            x[i] = (s0 + i < S) ? *(const f32x4*)(p.o_part + ((int64_t)(s0 + i) * rows + row) * d + c) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int i = 0; i < kKv8CombineBatch; ++i) {
            const float w = none ? 0.0f : __expf(l[s0 + i] - m);
            const bool live = w != 0.0f;   // an empty share never wrote its O: whatever was loaded is dropped
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = live ? __builtin_fmaf(w, x[i][e], acc[e]) : acc[e];
            wsum = live ? __builtin_fmaf(w, 1.0f, wsum) : wsum;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = none ? 0.0f : (acc[e] / wsum) * v_scale;
    if constexpr (OUT_F32) {
        *(f32x4*)((float*)p.o + row * d + c) = acc;
    } else {
        bf16x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = (__bf16)acc[e];
        *(bf16x4*)((__bf16*)p.o + row * d + c) = r;
    }
    if (p.lse != nullptr && c == 0) p.lse[row] = none ? -INFINITY : m + __logf(wsum);
}

hipError_t launch_kv8_combine(const Kv8Params& p8, int d, int out_f32, hipStream_t stream)
{
    const KvParams& p = p8.pg.kv;
    if (p.splits < 2 || p.splits > kKvMaxSplits) return hipErrorInvalidValue;
    const int64_t threads = (int64_t)p.bh_kv * p.m_rows * (d / 4);
    const int64_t blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (out_f32)
        hipLaunchKernelGGL(fa_kv8_combine_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, p, d, p8.v_scale);
    else
        hipLaunchKernelGGL(fa_kv8_combine_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, p, d, p8.v_scale);
    return hipGetLastError();
}

}  // namespace fa
