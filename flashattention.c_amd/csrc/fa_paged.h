// fa_paged.h -- what the translation units of libflashattn_amd_paged.so share (include/flashattn_amd_paged.h is the boundary).  The library is
// the KV-cache forward of fa_kv.h over a paged cache: the plan (kv_plan), the launch parameters of the merge (KvParams) and the merge kernel
// itself (fa_kv_combine.hip, compiled once and linked into both libraries) are that library's; the decode kernel is its own instance of the
// 16-bit loop (fa_kv_decode16_body.h).
#pragma once
#include "fa_kv.h"

namespace fa {

constexpr int kPagedMinPage = 16;          // rows: a 64-key block (kKvBlk, fa_bf16_common.h) spans at most 64 / 16 pages ...
constexpr int kPagedBlockPages = 64 / kPagedMinPage;   // ... whose table entries a wave holds as uniform values
constexpr int kPagedMaxPage = 65536;

struct PagedParams {
    KvParams kv;            // q, o, lse, the partials, the plan; k / v = the pools, kv_lens = seq_lens (one per SEQUENCE), bh_kv = batch * heads_kv
    const int32_t* table;   // device, [batch][max_pages]
    int64_t page_stride;    // elements
    int64_t head_stride;
    int32_t row_stride;     // elements; page_size * row_stride * 2 + head offset < 2^32 bytes
    int32_t max_pages;
    int32_t heads_kv;
    int32_t page_shift;     // log2(page_size)
};

hipError_t launch_paged_decode(const PagedParams& p, int d, int causal, int out_f32, hipStream_t stream);
const char* paged_decode_kernel_name();

}  // namespace fa
