// fa_kv8.h -- what the translation units of libflashattn_amd_kv8.so share (include/flashattn_amd_kv8.h is the boundary).  The library is the
// KV-cache forward of fa_kv.h / fa_paged.h over a cache of 8-bit floats (OCP e4m3fn): the plan (kv_plan) and the launch parameters are
// theirs; the decode kernel and the merge kernel (fa_kv_combine_kernel.h's body with the multiplication by v_scale) are its own.  It links no object of
// the other libraries.
#pragma once
#include "fa_paged.h"

namespace fa {

struct Kv8Params {
    PagedParams pg;   // contiguous cache: pg.kv alone (kv_slab_stride = capacity * d), the paged fields unused.  Strides in elements = bytes
    float v_scale;    // multiplies the normalised result once, before the store to o: in the decode kernel (unsplit) or in the merge (split)
};

hipError_t launch_kv8_decode(const Kv8Params& p, int d, int causal, int out_f32, int paged, hipStream_t stream);
hipError_t launch_kv8_combine(const Kv8Params& p, int d, int out_f32, hipStream_t stream);
const char* kv8_decode_kernel_name();

}  // namespace fa
