"""CPU: the host side of KV-cache attention over an fp8 cache (include/flashattn_amd_kv8.h, libflashattn_amd_kv8.so): the e4m3 table the GPU
tests build their reference with, the binding, argument validation (no device is touched before it passes), the plan -- that of the bf16
libraries -- and the code objects."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from flashattention_c_amd import _cabi_kv, _cabi_kv8
from tests import codeobj
from tests.kv8_reference import FP8_MAX, NAN_CODES, TABLE, dequant, quantize
from tests.test_kv_host import GRID, _family

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, 1, 2
BF16, BF16_F32, F32 = _cabi_kv8.FA_DTYPE_BF16, _cabi_kv8.FA_DTYPE_BF16_OUT_F32, _cabi_kv8.FA_DTYPE_F32


def test_the_table_is_torchs_e4m3fn_and_survives_bf16():
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    want = codes.view(torch.float8_e4m3fn).to(torch.float32).numpy().astype(np.float64)
    got = dequant(codes)
    nan = np.isnan(got)
    assert np.flatnonzero(nan).tolist() == list(NAN_CODES) and np.array_equal(np.isnan(want), nan)
    assert np.array_equal(got[~nan], want[~nan]) and np.array_equal(np.signbit(got[~nan]), np.signbit(want[~nan]))   # -0 at 0x80
    assert got[~nan].max() == FP8_MAX == -got[~nan].min() and np.count_nonzero(~nan) == 254
    # the arithmetic contract rests on this: every non-NaN value is a bf16 value
    through = torch.from_numpy(TABLE[~nan]).to(torch.bfloat16).to(torch.float64).numpy()
    assert np.array_equal(through, TABLE[~nan])
    assert np.array_equal(codes.view(torch.float8_e4m3fn).to(torch.bfloat16).to(torch.float64).numpy()[~nan], TABLE[~nan])
    # dequant takes the fp8 tensor itself too; quantize clamps and rounds as torch does
    assert np.array_equal(dequant(codes.view(torch.float8_e4m3fn))[~nan], TABLE[~nan])
    q = quantize(np.array([0.0, 1.0, 1000.0, -1000.0, 0.3]), 0.5)
    assert q.dtype == torch.float8_e4m3fn and dequant(q).tolist() == [0.0, 2.0, 448.0, -448.0, 0.625]


def test_header_prototypes_match_the_binding():
    hdr = open(os.path.join(ROOT, "include", "flashattn_amd_kv8.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(fa_kv8_[a-z_]+)\s*\(", hdr))
    assert declared == set(_cabi_kv8.EXPORTED_SYMBOLS), declared ^ set(_cabi_kv8.EXPORTED_SYMBOLS)
    L = _cabi_kv8.lib()
    for sym in declared:
        assert getattr(L, sym) is not None
    assert L.fa_kv8_version().startswith(b"flashattn_amd_kv8 abi 1 gfx950 ")
    exported = os.popen(f"nm -D --defined-only {_cabi_kv8.LIB_PATH}").read()
    assert set(re.findall(r" T (fa_\w+)", exported)) == declared
    assert not re.search(r" T fa_kv_| T fa_paged_", exported), "the fp8 library must not export the bf16 libraries' C symbols a second time"
    import flashattention_c_amd as fa
    from flashattention_c_amd import flash
    for name in ("forward_kv_fp8", "forward_paged_fp8"):
        assert name in fa.__all__ and name in flash.__all__ and callable(getattr(fa, name))


A = 0x7f0000000000   # pointers that are never dereferenced: validation comes before any device call
G = 1 << 30
Q, K, V, O, LSE, LENS, WS = A, A + 1 * G, A + 2 * G, A + 3 * G, A + 4 * G, A + 4 * G + (1 << 20), A + 5 * G


def _fwd(L, q=Q, k=K, v=V, o=O, lse=None, bh_kv=2, group=4, nq=1, nk=4096, cap=4096, lens=None, d=128, scale=1.0, k_scale=0.5, v_scale=2.0,
         causal=0, dtype=BF16, ws=None, ws_bytes=0):
    return L.fa_kv8_forward(q, k, v, o, lse, bh_kv, group, nq, nk, cap, lens, d, scale, k_scale, v_scale, causal, dtype, ws, ws_bytes, None)


BAD_SCALES = [0.0, -1.0, float("inf"), float("-inf"), float("nan")]


def test_validation_of_the_contiguous_entry_without_a_device():
    L = _cabi_kv8.lib()
    need = L.fa_kv8_workspace_bytes(2, 4, 1, 4096, 128, 0, BF16)
    assert need > 0
    slab = 4096 * 128                      # bytes of one K/V slab: an element is one byte
    rows = 2 * 4 * 1
    cases = [
        (dict(q=None), INVALID), (dict(k=None), INVALID), (dict(v=None), INVALID), (dict(o=None), INVALID),
        (dict(q=Q + 8), INVALID), (dict(k=K + 8), INVALID), (dict(v=V + 8), INVALID), (dict(o=O + 8), INVALID),
        (dict(lse=LSE + 2), INVALID), (dict(lens=LENS + 1), INVALID),
        (dict(nk=4097), INVALID),                                         # nk > capacity
        (dict(d=96), UNSUPPORTED), (dict(dtype=F32), UNSUPPORTED), (dict(dtype=7), INVALID),
        (dict(scale=0.0), INVALID), (dict(scale=float("nan")), INVALID), (dict(scale=float("inf")), INVALID),
        *[(dict(k_scale=s), INVALID) for s in BAD_SCALES], *[(dict(v_scale=s), INVALID) for s in BAD_SCALES],
        (dict(scale=1e30, k_scale=1e30), INVALID),                        # the fp32 product overflows ...
        (dict(scale=1e-30, k_scale=1e-30), INVALID),                      # ... or is zero
        (dict(cap=1 << 25), UNSUPPORTED),                                 # 2^25 * 128 = 2^32 bytes per slab
        (dict(nk=(1 << 24) + 1, cap=(1 << 24) + 1, d=64), UNSUPPORTED),
        (dict(group=0), INVALID), (dict(nq=0), INVALID), (dict(bh_kv=0), INVALID), (dict(nk=0), INVALID),
        # overlap: o against q, k8, v8 (the caches over their capacity, beyond the first nk rows too)
        (dict(o=Q), INVALID), (dict(nk=100, o=K + slab + 4000 * 128), INVALID), (dict(nk=100, o=V + 2 * slab - 16), INVALID),
        # ... lse against q, k8, v8, o
        (dict(lse=Q + 4), INVALID), (dict(lse=K + slab), INVALID), (dict(lse=V + 2 * slab - 4), INVALID), (dict(lse=O + rows * 128 * 2 - 4), INVALID),
        # ... the workspace against every tensor of the call
        (dict(ws=Q, ws_bytes=need), INVALID), (dict(ws=K + 2 * slab - 256, ws_bytes=need), INVALID), (dict(ws=V, ws_bytes=need), INVALID),
        (dict(ws=O, ws_bytes=need), INVALID), (dict(lse=WS + 256, ws=WS, ws_bytes=need), INVALID), (dict(lens=WS + 512, ws=WS, ws_bytes=need), INVALID),
        (dict(ws=WS, ws_bytes=need - 1), INVALID),                        # workspace too small
        (dict(ws=WS + 128, ws_bytes=need), INVALID),                      # ... misaligned
    ]
    for kw, code in cases:
        rc = _fwd(L, **kw)
        assert rc == code, (kw, rc, L.fa_kv8_last_error())
        assert L.fa_kv8_last_error(), kw
    assert _fwd(L, d=96) == UNSUPPORTED and b"64" in L.fa_kv8_last_error() and b"128" in L.fa_kv8_last_error()
    assert _fwd(L, k_scale=0.0) == INVALID and b"k_scale" in L.fa_kv8_last_error()
    assert _fwd(L, v_scale=float("nan")) == INVALID and b"v_scale" in L.fa_kv8_last_error()
    assert _fwd(L, scale=1e30, k_scale=1e30) == INVALID and b"scale * k_scale" in L.fa_kv8_last_error()
    assert _fwd(L, cap=1 << 25) == UNSUPPORTED and b"2^32" in L.fa_kv8_last_error()
    # the largest slab that passes does pass: the next check to fail is another one (the misaligned workspace)
    assert _fwd(L, cap=(1 << 25) - 1, v=A + 10 * G, o=A + 20 * G, ws=A + 30 * G + 128, ws_bytes=need) == INVALID and b"workspace" in L.fa_kv8_last_error()
    # a bf16 slab of that many BYTES would have been half the rows: the limit is in bytes, the capacity in elements
    assert _fwd(L, cap=1 << 24, v=A + 10 * G, o=A + 20 * G, ws=A + 30 * G + 128, ws_bytes=need) == INVALID and b"workspace" in L.fa_kv8_last_error()
    for args in ((2, 4, 1, 4096, 96, 0, BF16), (2, 4, 1, 4096, 128, 0, F32), (0, 4, 1, 4096, 128, 0, BF16), (2, 4, 1, (1 << 24) + 1, 128, 0, BF16)):
        assert L.fa_kv8_workspace_bytes(*args) == 0 and L.fa_kv8_splits_for(*args) == 0
        assert L.fa_kv8_kernel_name_for(*args, 0) is None and L.fa_kv8_kernel_name_for(*args, 64) is None


# the default paged call: 2 sequences x 2 heads, (pages, page, H, d) pools of 64 pages of 64 rows (1 MiB each, 16 KiB per page)
POOL_K, POOL_V, TABLE_P, LENS_P = A + 1 * G, A + 2 * G, A + 3 * G, A + 3 * G + (1 << 20)


def _paged(L, q=Q, o=A + 4 * G, lse=None, cache=True, batch=2, heads_kv=2, group=4, nq=1, nk=2048, d=128, scale=1.0, k_scale=0.5, v_scale=2.0, causal=0,
           dtype=BF16, ws=None, ws_bytes=0, **c):
    f = dict(k_pool=POOL_K, v_pool=POOL_V, num_pages=64, page_size=64, page_stride=64 * 2 * 128, row_stride=2 * 128, head_stride=128,
             block_table=TABLE_P, max_pages=32, seq_lens=LENS_P)
    f.update(c)
    cache = ctypes.byref(_cabi_kv8.FaPagedCache(**f)) if cache else None
    return L.fa_kv8_paged_forward(q, cache, o, lse, batch, heads_kv, group, nq, nk, d, scale, k_scale, v_scale, causal, dtype, ws, ws_bytes, None)


def test_validation_of_the_paged_entry_without_a_device():
    L = _cabi_kv8.lib()
    need = L.fa_kv8_workspace_bytes(2 * 2, 4, 1, 2048, 128, 0, BF16)
    assert need > 0
    page_bytes = 64 * 2 * 128
    o_bytes = 2 * 2 * 4 * 128 * 2
    OP = A + 4 * G
    cases = [
        (dict(q=None), INVALID), (dict(o=None), INVALID), (dict(cache=False), INVALID),
        (dict(k_pool=None), INVALID), (dict(v_pool=None), INVALID), (dict(block_table=None), INVALID),
        (dict(page_size=8), UNSUPPORTED), (dict(page_size=24), UNSUPPORTED), (dict(page_size=1 << 17, max_pages=1, row_stride=128, head_stride=0, heads_kv=1), UNSUPPORTED),
        (dict(page_stride=64 * 2 * 128 + 8), INVALID), (dict(row_stride=2 * 128 + 8), INVALID), (dict(head_stride=128 + 8), INVALID),   # multiples of 8: not enough
        (dict(page_stride=12), INVALID), (dict(row_stride=2 * 128 + 12), INVALID), (dict(head_stride=12), INVALID),
        (dict(row_stride=64, heads_kv=1, head_stride=0), INVALID),                # row_stride < d
        (dict(nk=2049), INVALID),                                               # nk > max_pages * page_size
        (dict(num_pages=0), INVALID), (dict(max_pages=0), INVALID),
        (dict(d=96), UNSUPPORTED), (dict(dtype=F32), UNSUPPORTED),
        (dict(scale=0.0), INVALID), (dict(scale=float("nan")), INVALID),
        *[(dict(k_scale=s), INVALID) for s in BAD_SCALES], *[(dict(v_scale=s), INVALID) for s in BAD_SCALES],
        (dict(scale=1e30, k_scale=1e30), INVALID), (dict(scale=1e-30, k_scale=1e-30), INVALID),
        (dict(q=Q + 8), INVALID), (dict(o=OP + 8), INVALID), (dict(k_pool=POOL_K + 8), INVALID), (dict(v_pool=POOL_V + 8), INVALID),
        (dict(lse=A + 6 * G + 2), INVALID), (dict(block_table=TABLE_P + 2), INVALID), (dict(seq_lens=LENS_P + 1), INVALID),
        # overlap: o, lse and the workspace against q, both pools over their whole strided extent, the table and the lengths
        (dict(o=Q), INVALID), (dict(o=POOL_K + 40 * page_bytes), INVALID), (dict(o=POOL_V + 63 * page_bytes + 1024), INVALID),
        (dict(o=TABLE_P), INVALID), (dict(o=LENS_P), INVALID),
        (dict(lse=Q + 4), INVALID), (dict(lse=POOL_K + 63 * page_bytes), INVALID), (dict(lse=POOL_V + 5 * page_bytes), INVALID),
        (dict(lse=TABLE_P + 4), INVALID), (dict(lse=LENS_P + 4), INVALID), (dict(lse=OP + o_bytes - 4), INVALID),
        (dict(ws=Q, ws_bytes=need), INVALID), (dict(ws=POOL_K + 63 * page_bytes, ws_bytes=need), INVALID), (dict(ws=POOL_V, ws_bytes=need), INVALID),
        (dict(ws=TABLE_P, ws_bytes=need), INVALID),                               # workspace over the table
        (dict(ws=TABLE_P + 256, ws_bytes=need, max_pages=4096, nk=2048), INVALID),  # ... over its second row
        (dict(ws=LENS_P - 256, ws_bytes=need), INVALID),                          # ... over the lengths
        (dict(ws=OP, ws_bytes=need), INVALID), (dict(lse=WS + 256, ws=WS, ws_bytes=need), INVALID),
        (dict(ws=WS, ws_bytes=need - 1), INVALID),                                # workspace too small
        (dict(ws=WS + 128, ws_bytes=need), INVALID),                              # ... misaligned
        (dict(page_size=65536, max_pages=1, row_stride=65536, page_stride=1 << 32, heads_kv=1, head_stride=0, batch=4), UNSUPPORTED),   # 2^32 bytes inside a page
        (dict(page_size=65536, max_pages=1, row_stride=65536 - 16, page_stride=1 << 32, heads_kv=2, head_stride=65536 * 16), UNSUPPORTED),   # ... by the head offset
        (dict(nk=(1 << 24) + 1, page_size=65536, max_pages=512), UNSUPPORTED),
        (dict(group=0), INVALID), (dict(nq=0), INVALID), (dict(batch=0), INVALID), (dict(heads_kv=0), INVALID),
    ]
    for kw, code in cases:
        rc = _paged(L, **kw)
        assert rc == code, (kw, rc, L.fa_kv8_last_error())
        assert L.fa_kv8_last_error(), kw
    assert _paged(L, page_size=24) == UNSUPPORTED and b"power of two" in L.fa_kv8_last_error()
    assert _paged(L, nk=2049) == INVALID and b"max_pages" in L.fa_kv8_last_error()
    assert _paged(L, row_stride=2 * 128 + 8) == INVALID and b"multiples of 16" in L.fa_kv8_last_error()
    assert LENS_P - 256 + need > LENS_P   # the case above does reach the lengths
    # the largest in-page extent that passes validation does pass it: the next check to fail is another one (here: the misaligned workspace)
    assert _paged(L, page_size=65536, max_pages=1, row_stride=65536 - 16, page_stride=1 << 32, heads_kv=1, head_stride=0, batch=4, num_pages=1,
                  ws=WS + 128, ws_bytes=need) == INVALID
    assert b"workspace" in L.fa_kv8_last_error()
    for page in (8, 24, 1 << 17, -16):
        assert L.fa_kv8_kernel_name_for(4, 4, 1, 2048, 128, 0, BF16, page) is None
    assert L.fa_kv8_kernel_name_for(4, 4, 1, 2048, 128, 0, BF16, 16) == L.fa_kv8_kernel_name_for(4, 4, 1, 2048, 128, 0, BF16, 0) == b"fa_kv8_decode_kernel"


def test_the_plan_is_the_kv_librarys_over_the_grid():
    L, K8 = _cabi_kv.lib(), _cabi_kv8.lib()
    split = 0
    for bh_kv, group, nq, nk, d in GRID:
        for causal, dt in ((0, BF16), (1, BF16_F32)):
            what = (bh_kv, group, nq, nk, d, causal, dt)
            S = K8.fa_kv8_splits_for(*what)
            assert S >= 1 and S == L.fa_kv_splits_for(*what), what
            assert K8.fa_kv8_workspace_bytes(*what) == L.fa_kv_workspace_bytes(*what), what
            split += S > 1
    assert split > 100


@pytest.fixture(scope="module")
def kv8_kernels(tmp_path_factory):
    assert os.path.exists(_cabi_kv8.LIB_PATH), "build the library first (python flashattention.c_amd/build.py)"
    return codeobj.kernels_of(_cabi_kv8.LIB_PATH, str(tmp_path_factory.mktemp("co_kv8")))


def test_code_objects_of_the_fp8_library(kv8_kernels, tmp_path):
    spilling = [f"{k.scratch} B: {k.name}" for k in kv8_kernels.values() if k.scratch != 0]
    assert not spilling, "\n".join(spilling)
    L = _cabi_kv8.lib()
    reachable = set()
    for bh_kv, group, nq, nk, d in GRID:
        for causal, dt in ((0, BF16), (1, BF16_F32)):
            for page in (0, 16, 32, 64, 256, 65536):
                reachable.add(L.fa_kv8_kernel_name_for(bh_kv, group, nq, nk, d, causal, dt, page).decode())
    present = {_family(k.name) for k in kv8_kernels.values()}
    assert present == reachable | {"fa_kv8_combine_kernel"}, present ^ (reachable | {"fa_kv8_combine_kernel"})
    # every instantiation the launcher can pick: d x causal x output type x (contiguous, paged)
    decode = [k for k in kv8_kernels.values() if "fa_kv8_decode_kernel<" in k.name]
    assert len(decode) == 16 and len(kv8_kernels) == 18, sorted(k.name for k in kv8_kernels.values())
    # LDS: no more than the bf16 kernel of the same d takes (one V image per wave instead of two)
    kv = codeobj.kernels_of(_cabi_kv.LIB_PATH, str(tmp_path))
    kv_lds = {re.search(r"<(\d+),", k.name).group(1): k.lds for k in kv.values() if "fa_kv_decode_kernel<" in k.name}
    assert set(kv_lds) == {"64", "128"}
    for k in decode:
        assert 0 < k.lds <= kv_lds[re.search(r"<(\d+),", k.name).group(1)], (k.name, k.lds, kv_lds)
