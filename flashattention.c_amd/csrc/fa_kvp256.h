// fa_kvp256.h -- what the translation units of libflashattn_amd_kvp256.so share (include/flashattn_amd_kvp256.h is the boundary): the launch
// parameters of the chunked-prefill kernels at head dim 256 and their launcher.  The library is fa_kvp.h's at d = 256: validation and the fill
// of the parameters are fa_kv_host.h's (the unsplit plan: no key split, no workspace), the kernel is its own (fa_kvp256_prefill_loop.h),
// because the two row blocks per wave of fa_kvp_prefill_loop.h alone would fill the accumulation half of the register file at this width.
// Under a sliding window: fa_kvpw.h, libflashattn_amd_kvpw.so.  Out of scope: fp8 caches, a key split for tiny grids, routing from fa_kv256_forward.
#pragma once
#include "fa_paged.h"

namespace fa {

constexpr int kKvp256HeadDim = 256;
constexpr int kKvp256RowTile = 128;   // packed query rows per workgroup: four waves x one 32-row MFMA block column

// One by-value argument for the eight kernels: a contiguous cache fills pp.kv and leaves the page fields zero (never read with PAGED = false).
// Of the plan in pp.kv only m_rows, nq, nk and bh_kv are read: row_tiles, splits and share are those of the decode kernels' 32-row tiles.
struct Kvp256Params {
    PagedParams pp;
    int32_t tiles;   // ceil(group * nq / kKvp256RowTile): the launch has bh_kv * tiles workgroups
};

hipError_t launch_kvp256_prefill(const Kvp256Params& p, int paged, int causal, int out_f32, hipStream_t stream);
const char* kvp256_prefill_kernel_name();

}  // namespace fa
