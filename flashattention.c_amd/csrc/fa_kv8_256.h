// fa_kv8_256.h -- what the translation units of libflashattn_amd_kv8_256.so share (include/flashattn_amd_kv8_256.h is the boundary): the launch
// parameters of the head-dim-256 decode kernels over an fp8 (e4m3fn) cache and their launcher.  The library is fa_kv256.h's with the cache of
// fa_kv8.h: plan (kv_plan, over kvw_span where a window bounds the keys) and window check are fa_kvw.h's, the merge kernel is the object of
// fa_kv8_combine.hip (d at run time, the multiplication by v_scale); the decode kernel is its own (fa_kv8_256_decode_loop.h).
#pragma once
#include "fa_kv256.h"
#include "fa_kv8.h"

namespace fa {

// One by-value argument for the sixteen kernels: Kv8Params as the merge kernel takes it, the window beside it
struct Kv8x256Params {
    Kv8Params k8;          // a contiguous cache fills k8.pg.kv and leaves the page fields zero (never read with PAGED = false)
    int32_t window_left;   // 0 .. kKvwMaxWindow where the kernel is a WINDOW one; not read otherwise
};

hipError_t launch_kv8_256_decode(const Kv8x256Params& p, int paged, int window, int causal, int out_f32, hipStream_t stream);
const char* kv8_256_decode_kernel_name();

}  // namespace fa
