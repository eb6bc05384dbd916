// fa_kv_combine_kernel.h -- the merge of a key-split KV-cache forward: S <= 64 workgroups per row tile left normalised fp32 partial outputs
// O_s ([S][rows][d]) and the log-sum-exp of their share (natural log, [S][rows]; -inf: the share held no key this row sees, and its O_s
// may never have been written) in the workspace.  O = sum_s w_s O_s / sum_s w_s with w_s = exp(lse_s - max_s lse_s); LSE = max +
// log(sum_s w_s); a row whose shares are all -inf gets O = 0 and LSE = -inf (fa_combine.hip of the product library would form
// exp(-inf - -inf) there and stops at 8 shares, which is why these libraries have their own).
// One thread per four output columns.  As in fa_combine.hip every load is issued before the first is used: all S log-sum-exps at
// once, the partial outputs in batches of 16 (four dependent round trips at S = 64 instead of 64).
//
// SCALED (the fp8 cache, fa_kv8_combine.hip): ONE more operation, the multiplication of the merged, normalised row by v_scale in front of
// the store.  Why the key shares do not store partial outputs that are scaled already: the merge forms sum_s w_s O_s / sum_s w_s with one
// fused multiply-add per share in the numerator and the same sequence against 1 in the denominator; the quotient of the two is exact where
// every O_s is 1 (a constant V), and off by a few ulp where every O_s is fp32(0.37) -- measured: 512 of 1024 elements, up to 3 ulp, at
// 1 x 8 x 1 x 8192 x 128.  With the scale applied here, behind the quotient, a constant V comes out as fp32(v_scale * constant) from split
// launches as it does from unsplit ones, and everything in front of it is the unscaled merge instruction for instruction: with v_scale a
// power of two the result is still v_scale x the bf16 library's, bit for bit.
#pragma once
#include "fa_kv.h"

namespace fa {

constexpr int kKvCombineBatch = 16;

// the body of a __global__ __launch_bounds__(256) kernel; v_scale is read only where SCALED
template <bool OUT_F32, bool SCALED>
__device__ __forceinline__ void kv_combine_body(const KvParams& p, int d, float v_scale)
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
    for (int s0 = 0; s0 < kKvMaxSplits; s0 += kKvCombineBatch) {
        if (s0 >= S) break;   // uniform
        f32x4 x[kKvCombineBatch];
#pragma unroll
        for (int i = 0; i < kKvCombineBatch; ++i)
            x[i] = (s0 + i < S) ? *(const f32x4*)(p.o_part + ((int64_t)(s0 + i) * rows + row) * d + c) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int i = 0; i < kKvCombineBatch; ++i) {
            const float w = none ? 0.0f : __expf(l[s0 + i] - m);
            const bool live = w != 0.0f;   // an empty share never wrote its O: whatever was loaded is dropped
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = live ? __builtin_fmaf(w, x[i][e], acc[e]) : acc[e];
            wsum = live ? __builtin_fmaf(w, 1.0f, wsum) : wsum;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if constexpr (SCALED)
            acc[e] = none ? 0.0f : (acc[e] / wsum) * v_scale;
        else
            acc[e] = none ? 0.0f : acc[e] / wsum;
    }
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

// grid of the merge, or 0: the launch is not possible
inline unsigned kv_combine_blocks(const KvParams& p, int d)
{
    if (p.splits < 2 || p.splits > kKvMaxSplits) return 0;
    const int64_t threads = (int64_t)p.bh_kv * p.m_rows * (d / 4);
    const int64_t blocks = (threads + 255) / 256;
    return blocks > 0x7fffffffLL ? 0u : (unsigned)blocks;
}

}  // namespace fa
