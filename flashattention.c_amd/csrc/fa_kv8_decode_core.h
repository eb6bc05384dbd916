// fa_kv8_decode_core.h -- what the fp8 decode loop (fa_kv8_decode_body.h) needs at namespace scope: the geometry of a wave's block, the exact
// e4m3 -> bf16 conversion and the swizzle of the V image.  Users: fa_kv8_decode.hip and fa_kvw8_decode.hip.
#pragma once
#include "fa_kv_decode_core.h"

namespace fa {

typedef __attribute__((ext_vector_type(2))) float f32x2;

template <int D>
struct Kv8Cfg {
    static constexpr int KS = D / 16, DB = D / 32;
    static constexpr int LPR = D / 16;                     // lanes per V row: 16 bytes (16 columns) each
    static constexpr int kVLoads = kKvBlk * D / 1024;      // 16-byte V loads per lane and block
    static constexpr int kRowsPerLoad = kWave / LPR;       // keys one V load instruction covers
    static constexpr int kVTile = kKvBlk * 2 * D;          // bytes of the V image (64 keys, bf16)
    static constexpr int kMergeBytes = kKvRowTile * kKvMergeStride(D) * 4;
    static constexpr int kWaveLds = kVTile > kMergeBytes ? kVTile : kMergeBytes;   // one image per wave, reused by the merge
    static_assert(kPagedMinPage % kRowsPerLoad == 0, "a V load must not straddle a 16-key group");
    static_assert(kWaveLds % 128 == 0, "sub-tile alignment");
};

// 8 e4m3 bytes (two dwords, ascending columns) -> 8 bf16, exactly
__device__ __forceinline__ bf16x8 cvt_fp8x8(unsigned lo, unsigned hi)
{
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8(lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8(lo, true);
    const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8(hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8(hi, true);
    bf16x8 r;
    r[0] = (__bf16)a[0], r[1] = (__bf16)a[1], r[2] = (__bf16)b[0], r[3] = (__bf16)b[1];
    r[4] = (__bf16)c[0], r[5] = (__bf16)c[1], r[6] = (__bf16)d[0], r[7] = (__bf16)d[1];
    return r;
}

// byte offset in the V image -> where it is kept: the 16-byte slot (bits 4 .. 6) XOR a code of the sub-tile's column block
// (fa_kv8_decode_body.h says why)
template <int D>
__device__ __forceinline__ int v_swz(int off)
{
    constexpr int LPR = D / 16;
    const int cb = (off >> 7) % LPR;
    const int g = LPR == 8 ? cb : ((cb & 1) | ((cb & 2) << 1));
    return off ^ (g << 4);
}

}  // namespace fa
