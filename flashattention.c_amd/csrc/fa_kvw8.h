// fa_kvw8.h -- what the translation units of libflashattn_amd_kvw8.so share (include/flashattn_amd_kvw8.h is the boundary): the launch
// parameters of the sliding-window fp8 decode kernel and its launcher.  The library is the fp8 KV-cache forward of fa_kv8.h with the lower
// bound of fa_kvw.h on the keys a query row sees: the plan (kv_plan over kvw_span) and the window's check are fa_kvw.h's, the merge kernel is
// the object of fa_kv8_combine.hip, the decode kernel is its own instance of the fp8 loop (fa_kv8_decode_body.h with WINDOW = true).
#pragma once
#include "fa_kv8.h"
#include "fa_kvw.h"

namespace fa {

// Kv8Params is the by-value argument of every kernel of libflashattn_amd_kv8.so and stays as it is: the window travels beside it
struct Kvw8Params {
    Kv8Params k8;
    int32_t window_left;   // query i sees keys j >= len - nq + i - window_left; 0 .. kKvwMaxWindow
};

hipError_t launch_kvw8_decode(const Kvw8Params& p, int d, int causal, int out_f32, int paged, hipStream_t stream);
const char* kvw8_decode_kernel_name();

}  // namespace fa
