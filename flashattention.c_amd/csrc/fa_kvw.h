// fa_kvw.h -- what the translation units of libflashattn_amd_kvw.so share (include/flashattn_amd_kvw.h is the boundary): the launch parameters
// of the sliding-window decode kernels and their launchers.  The library is the KV-cache forward of fa_kv.h / fa_paged.h with a lower bound
// on the keys a query row sees: the plan (kv_plan, over the widest key range a row tile can have), the parameters of the merge (KvParams)
// and the merge kernel (the object of fa_kv_combine.hip) are those libraries'; the decode kernels are its own instances of the 16-bit loop
// (fa_kv_decode16_body.h with WINDOW = true).
#pragma once
#include "fa_paged.h"

namespace fa {

constexpr int32_t kKvwMaxWindow = 1 << 24;   // = the largest nk: a wider window hides no key

// KvParams / PagedParams are the by-value argument of every kernel of the other libraries and stay as they are: the window travels beside them
struct KvwParams {
    KvParams kv;
    int32_t window_left;   // query i sees keys j >= len - nq + i - window_left; 0 .. kKvwMaxWindow
};
struct KvwPagedParams {
    PagedParams pp;
    int32_t window_left;
};

// The widest key range [lo & ~63, upper) a row tile can have: window_left + nq keys from the lowest row's first key to the slab's end, plus
// the up to 63 keys down to the block boundary.  The plan runs over it, so share * splits covers every tile whatever the lengths are.
inline int64_t kvw_span(int64_t nq, int64_t nk, int32_t window_left)
{
    const int64_t span = (int64_t)window_left + nq + 63;
    return span < nk ? span : nk;
}

hipError_t launch_kvw_decode(const KvwParams& p, int d, int causal, int out_f32, hipStream_t stream);
hipError_t launch_kvw_paged_decode(const KvwPagedParams& p, int d, int causal, int out_f32, hipStream_t stream);
const char* kvw_decode_kernel_name();
const char* kvw_paged_decode_kernel_name();

}  // namespace fa
