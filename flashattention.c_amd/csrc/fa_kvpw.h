// fa_kvpw.h -- what the translation units of libflashattn_amd_kvpw.so share (include/flashattn_amd_kvpw.h is the boundary): the launch
// parameters of the chunked-prefill kernels under a sliding window and their launchers.  The library is those of fa_kvp.h, fa_kvp8.h and
// fa_kvp256.h with the lower bound of fa_kvw.h on the keys a query row sees: validation and the fill of the parameters are fa_kv_host.h's
// (the unsplit plan, no workspace; the window checked by check_window), the kernels are the two prefill loops compiled with WINDOW = true
// (fa_kvp_prefill_loop.h at d = 128, bf16 and fp8; fa_kvp256_prefill_loop.h at d = 256, bf16).
#pragma once
#include "fa_kvp.h"
#include "fa_kvp256.h"
#include "fa_kvp8.h"

namespace fa {

// KvpParams, Kvp8Params and Kvp256Params are the by-value arguments of the unwindowed kernels and stay as they are: the window travels
// beside them (query i sees keys j >= len - nq + i - window_left; 0 .. kKvwMaxWindow)
struct KvpwParams {
    KvpParams p;
    int32_t window_left;
};
struct Kvpw8Params {
    Kvp8Params p;
    int32_t window_left;
};
struct Kvpw256Params {
    Kvp256Params p;
    int32_t window_left;
};

hipError_t launch_kvpw_prefill(const KvpwParams& wp, int paged, int causal, int out_f32, hipStream_t stream);
hipError_t launch_kvpw8_prefill(const Kvpw8Params& wp, int paged, int causal, int out_f32, hipStream_t stream);
hipError_t launch_kvpw256_prefill(const Kvpw256Params& wp, int paged, int causal, int out_f32, hipStream_t stream);

}  // namespace fa
