// fa_kvp8.h -- what the translation units of libflashattn_amd_kvp8.so share (include/flashattn_amd_kvp8.h is the boundary): the launch
// parameters of the chunked-prefill kernels over a cache of 8-bit floats (OCP e4m3fn) and their launcher.  The library is fa_kvp.h's with the
// cache of fa_kv8.h: validation and the fill of the parameters are fa_kv_host.h's with an element of one byte, the kernel is
// fa_kvp_prefill_loop.h compiled with FP8 = true, which replaces the LDS-DMA of a block by loads, an exact conversion and LDS stores.
#pragma once
#include "fa_kvp.h"

namespace fa {

// KvpParams and the scale of V.  Strides of the cache in elements = bytes.
struct Kvp8Params {
    PagedParams pp;
    int32_t tiles;    // ceil(group * nq / kKvpRowTile): the launch has bh_kv * tiles workgroups
    float v_scale;    // multiplies the normalised result once, before the store to o
};

hipError_t launch_kvp8_prefill(const Kvp8Params& p, int paged, int causal, int out_f32, hipStream_t stream);
const char* kvp8_prefill_kernel_name();

}  // namespace fa
