// fa_kvp.h -- what the translation units of libflashattn_amd_kvp.so share (include/flashattn_amd_kvp.h is the boundary): the launch parameters
// of the chunked-prefill kernels and their launcher.  The library is the KV-cache forward of fa_kv.h / fa_paged.h for MANY query rows at
// d = 128: validation and the fill of the parameters are fa_kv_host.h's (the unsplit plan: there is no key split here and no workspace), the
// kernel is its own (fa_kvp_prefill_loop.h), because the decode loop re-reads the K/V slab once per 32 rows.
// Under a sliding window: fa_kvpw.h, libflashattn_amd_kvpw.so.  Out of scope (fp8 caches: fa_kvp8.h, libflashattn_amd_kvp8.so): d = 64 (d = 256: fa_kvp256.h, libflashattn_amd_kvp256.so), a key split for tiny grids, routing from fa_kv_forward.
#pragma once
#include "fa_paged.h"

namespace fa {

constexpr int kKvpHeadDim = 128;
constexpr int kKvpRowTile = 256;   // packed query rows per workgroup: four waves x two 32-row MFMA block columns

// One by-value argument for the eight kernels: a contiguous cache fills pp.kv and leaves the page fields zero (never read with PAGED = false).
// Of the plan in pp.kv only m_rows, nq, nk and bh_kv are read: row_tiles, splits and share are those of the decode kernels' 32-row tiles.
struct KvpParams {
    PagedParams pp;
    int32_t tiles;   // ceil(group * nq / kKvpRowTile): the launch has bh_kv * tiles workgroups
};

hipError_t launch_kvp_prefill(const KvpParams& p, int paged, int causal, int out_f32, hipStream_t stream);
const char* kvp_prefill_kernel_name();

}  // namespace fa
