// fa_kv256.h -- what the translation units of libflashattn_amd_kv256.so share (include/flashattn_amd_kv256.h is the boundary): the launch
// parameters of the head-dim-256 decode kernels and their launchers.  The library is the KV-cache forward of fa_kv.h / fa_paged.h / fa_kvw.h at
// d = 256: the plan (kv_plan, over kvw_span where a window bounds the keys), the parameters of the merge (KvParams) and the merge kernel (the
// object of fa_kv_combine.hip, which takes d at run time) are those libraries'; the decode kernel is its own (fa_kv256_decode_loop.h), because
// the 64-key block of fa_kv_decode16_body.h fits neither the LDS, nor the 6-bit load counter, nor the register file at this width.
#pragma once
#include "fa_kvw.h"

namespace fa {

constexpr int kKv256HeadDim = 256;

// One by-value argument for the sixteen kernels: a contiguous cache fills pp.kv and leaves the page fields zero (never read with PAGED = false)
struct Kv256Params {
    PagedParams pp;
    int32_t window_left;   // 0 .. kKvwMaxWindow where the kernel is a WINDOW one; not read otherwise
};

hipError_t launch_kv256_decode(const Kv256Params& p, int paged, int window, int causal, int out_f32, hipStream_t stream);
const char* kv256_decode_kernel_name();

}  // namespace fa
