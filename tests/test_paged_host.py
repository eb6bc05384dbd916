"""CPU: the host side of paged KV-cache attention (include/flashattn_amd_paged.h, libflashattn_amd_paged.so): the gather the GPU tests build their
reference with, the binding, argument validation (no device is touched before it passes), the plan -- that of the contiguous-cache library --
and the code objects."""
import ctypes
import os
import re

import numpy as np
import pytest

from flashattention_c_amd import _cabi_kv, _cabi_paged
from tests import codeobj
from tests.kv_reference import attention_kv
from tests.paged_reference import gather
from tests.test_kv_host import GRID, _family

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, 1, 2
BF16, BF16_F32, F32 = _cabi_paged.FA_DTYPE_BF16, _cabi_paged.FA_DTYPE_BF16_OUT_F32, _cabi_paged.FA_DTYPE_F32


def test_gather_on_a_hand_written_example():
    # 3 pages of 2 rows, d = 1: page p holds rows 10 p, 10 p + 1
    pool = np.array([[[0.], [1.]], [[10.], [11.]], [[20.], [21.]]])
    table = np.array([[2, 0], [1, 99]])          # sequence 1 has one page; its second entry is never looked at
    got = gather(pool, table, [3, 2])
    assert got.shape == (2, 3, 1)
    assert got[:, :, 0].tolist() == [[20., 21., 0.], [10., 11., 0.]]   # rows past a sequence's length: zero
    assert gather(pool, table, [4, 1], nk=4)[:, :, 0].tolist() == [[20., 21., 0., 1.], [10., 0., 0., 0.]]
    # (pages, page, H, d): slab b * H + h
    pool4 = np.stack([pool, pool + 100.], axis=2)
    got4 = gather(pool4, table, [3, 2])
    assert got4.shape == (4, 3, 1)
    assert got4[:, :, 0].tolist() == [[20., 21., 0.], [120., 121., 100.], [10., 11., 0.], [110., 111., 0.]]
    with pytest.raises(AssertionError):
        gather(pool, table, [3, 3])               # would dereference the entry 99
    # the reference result: attention over the gathered cache, each sequence at its own length
    q = np.ones((2, 1, 1))
    o, lse = attention_kv(q, got, got, [3, 2], False, 1.0)
    w = np.exp([20., 21., 0.])
    assert abs(o[0, 0, 0] - (w * [20., 21., 0.]).sum() / w.sum()) < 1e-12 and abs(lse[1, 0] - np.log(np.exp(10.) + np.exp(11.))) < 1e-12


def test_header_prototypes_match_the_binding():
    hdr = open(os.path.join(ROOT, "include", "flashattn_amd_paged.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(fa_paged_[a-z_]+)\s*\(", hdr))
    assert declared == set(_cabi_paged.EXPORTED_SYMBOLS), declared ^ set(_cabi_paged.EXPORTED_SYMBOLS)
    L = _cabi_paged.lib()
    for sym in declared:
        assert getattr(L, sym) is not None
    assert b"gfx950" in L.fa_paged_version() and b"abi 1" in L.fa_paged_version()
    fields = re.search(r"typedef struct fa_paged_cache \{(.*?)\} fa_paged_cache;", hdr, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [n for n, _ in _cabi_paged.FaPagedCache._fields_]
    exported = os.popen(f"nm -D --defined-only {_cabi_paged.LIB_PATH}").read()
    assert not re.search(r" T fa_kv_", exported), "the paged library must not export the KV library's C symbols a second time"
    import flashattention_c_amd as fa
    assert "forward_paged" in fa.__all__ and "workspace_bytes_paged" in fa.__all__ and callable(fa.forward_paged)


A = 0x7f0000000000   # pointers that are never dereferenced: validation comes before any device call
G = 1 << 30
# the default call: 2 sequences x 2 heads, (pages, page, H, d) pools of 64 pages of 64 rows (2 MiB each, 32 KiB per page)
POOL_K, POOL_V, TABLE, LENS, Q, O, WS = A + 1 * G, A + 2 * G, A + 3 * G, A + 3 * G + (1 << 20), A, A + 4 * G, A + 5 * G


def _fwd(L, q=Q, o=O, lse=None, cache=True, batch=2, heads_kv=2, group=4, nq=1, nk=2048, d=128, scale=1.0, causal=0, dtype=BF16, ws=None, ws_bytes=0, **c):
    f = dict(k_pool=POOL_K, v_pool=POOL_V, num_pages=64, page_size=64, page_stride=64 * 2 * 128, row_stride=2 * 128, head_stride=128,
             block_table=TABLE, max_pages=32, seq_lens=LENS)
    f.update(c)
    cache = ctypes.byref(_cabi_paged.FaPagedCache(**f)) if cache else None
    return L.fa_paged_forward(q, cache, o, lse, batch, heads_kv, group, nq, nk, d, scale, causal, dtype, ws, ws_bytes, None)


def test_validation_without_a_device():
    L = _cabi_paged.lib()
    need = L.fa_paged_workspace_bytes(2, 2, 4, 1, 2048, 128, 0, BF16)
    assert need > 0
    page_bytes = 64 * 2 * 128 * 2
    cases = [
        (dict(q=None), INVALID), (dict(o=None), INVALID), (dict(cache=False), INVALID),
        (dict(k_pool=None), INVALID), (dict(v_pool=None), INVALID), (dict(block_table=None), INVALID),
        (dict(page_size=8), UNSUPPORTED), (dict(page_size=24), UNSUPPORTED), (dict(page_size=1 << 17, max_pages=1, row_stride=128, head_stride=0, heads_kv=1), UNSUPPORTED),
        (dict(page_stride=12), INVALID), (dict(row_stride=2 * 128 + 12), INVALID), (dict(head_stride=12), INVALID),
        (dict(row_stride=64, heads_kv=1, head_stride=0), INVALID),                # row_stride < d
        (dict(nk=2049), INVALID),                                               # nk > max_pages * page_size
        (dict(num_pages=0), INVALID), (dict(max_pages=0), INVALID),
        (dict(d=96), UNSUPPORTED), (dict(dtype=F32), UNSUPPORTED),
        (dict(scale=0.0), INVALID), (dict(scale=float("nan")), INVALID),
        (dict(q=Q + 8), INVALID), (dict(k_pool=POOL_K + 8), INVALID), (dict(block_table=TABLE + 2), INVALID), (dict(seq_lens=LENS + 1), INVALID),
        (dict(o=POOL_K + 40 * page_bytes), INVALID),                              # o inside the K pool's extent, far beyond its first page
        (dict(o=POOL_V + 63 * page_bytes + 1024), INVALID),                       # ... and inside the last page of the V pool
        (dict(lse=POOL_V + 5 * page_bytes), INVALID),
        (dict(ws=TABLE, ws_bytes=need), INVALID),                                 # workspace over the table
        (dict(ws=TABLE + 256, ws_bytes=need, max_pages=4096, nk=2048), INVALID),  # ... over its second row
        (dict(ws=POOL_K + 63 * page_bytes, ws_bytes=need), INVALID),              # ... over the last page of a pool
        (dict(ws=O, ws_bytes=need), INVALID),                                     # ... over o
        (dict(ws=A + 5 * G, ws_bytes=need - 1), INVALID),                         # workspace too small
        (dict(ws=A + 5 * G + 128, ws_bytes=need), INVALID),                       # ... misaligned
        (dict(page_size=65536, max_pages=1, row_stride=32768, page_stride=1 << 31, heads_kv=1, head_stride=0, batch=4), UNSUPPORTED),   # 2^32 bytes inside a page
        (dict(page_size=65536, max_pages=1, row_stride=32768 - 8, page_stride=1 << 31, heads_kv=2, head_stride=65536 * 8), UNSUPPORTED),   # ... by the head offset
        (dict(nk=(1 << 24) + 1, page_size=65536, max_pages=512), UNSUPPORTED),
        (dict(group=0), INVALID), (dict(nq=0), INVALID), (dict(batch=0), INVALID), (dict(heads_kv=0), INVALID),
    ]
    for kw, code in cases:
        rc = _fwd(L, **kw)
        assert rc == code, (kw, rc, L.fa_paged_last_error())
        assert L.fa_paged_last_error(), kw
    assert _fwd(L, page_size=24) == UNSUPPORTED and b"power of two" in L.fa_paged_last_error()
    assert _fwd(L, nk=2049) == INVALID and b"max_pages" in L.fa_paged_last_error()
    # the largest in-page extent that passes validation does pass it: the next check to fail is another one (here: the misaligned workspace)
    assert _fwd(L, page_size=65536, max_pages=1, row_stride=32768 - 8, page_stride=1 << 31, heads_kv=1, head_stride=0, batch=4, ws=A + 5 * G + 128, ws_bytes=need) == INVALID
    assert b"workspace" in L.fa_paged_last_error()
    for args in ((2, 2, 4, 1, 2048, 96, 0, BF16), (2, 2, 4, 1, 2048, 128, 0, F32), (0, 2, 4, 1, 2048, 128, 0, BF16), (2, 0, 4, 1, 2048, 128, 0, BF16),
                 (2, 2, 4, 1, (1 << 24) + 1, 128, 0, BF16)):
        assert L.fa_paged_workspace_bytes(*args) == 0 and L.fa_paged_splits_for(*args) == 0 and L.fa_paged_kernel_name_for(*args, 64) is None
    for page in (8, 24, 1 << 17, 0, -16):
        assert L.fa_paged_kernel_name_for(2, 2, 4, 1, 2048, 128, 0, BF16, page) is None
    assert L.fa_paged_kernel_name_for(2, 2, 4, 1, 2048, 128, 0, BF16, 16) == b"fa_paged_decode_kernel"


def test_the_plan_is_the_kv_librarys_over_the_grid():
    L, K = _cabi_paged.lib(), _cabi_kv.lib()
    split = 0
    for bh_kv, group, nq, nk, d in GRID:
        for heads_kv in {1, 2, 4, bh_kv} - {h for h in (2, 4) if bh_kv % h}:
            batch = bh_kv // heads_kv
            for causal, dt in ((0, BF16), (1, BF16_F32)):
                what = (batch, heads_kv, group, nq, nk, d, causal, dt)
                S = L.fa_paged_splits_for(*what)
                assert S >= 1 and S == K.fa_kv_splits_for(bh_kv, group, nq, nk, d, causal, dt), what
                assert L.fa_paged_workspace_bytes(*what) == K.fa_kv_workspace_bytes(bh_kv, group, nq, nk, d, causal, dt), what
                split += S > 1
    assert split > 100
    # the same bh_kv split two ways
    assert L.fa_paged_splits_for(8, 1, 8, 1, 8192, 128, 0, BF16) == L.fa_paged_splits_for(2, 4, 8, 1, 8192, 128, 0, BF16) == K.fa_kv_splits_for(8, 8, 1, 8192, 128, 0, BF16) > 1


@pytest.fixture(scope="module")
def paged_kernels(tmp_path_factory):
    assert os.path.exists(_cabi_paged.LIB_PATH), "build the library first (python flashattention.c_amd/build.py)"
    return codeobj.kernels_of(_cabi_paged.LIB_PATH, str(tmp_path_factory.mktemp("co_paged")))


def test_code_objects_of_the_paged_library(paged_kernels, tmp_path):
    spilling = [f"{k.scratch} B: {k.name}" for k in paged_kernels.values() if k.scratch != 0]
    assert not spilling, "\n".join(spilling)
    L = _cabi_paged.lib()
    reachable = set()
    for bh_kv, group, nq, nk, d in GRID:
        for causal, dt in ((0, BF16), (1, BF16_F32)):
            for page in (16, 32, 64, 256, 65536):
                reachable.add(L.fa_paged_kernel_name_for(bh_kv, 1, group, nq, nk, d, causal, dt, page).decode())
    present = {_family(k.name) for k in paged_kernels.values()}
    assert present == reachable | {"fa_kv_combine_kernel"}, present ^ (reachable | {"fa_kv_combine_kernel"})
    decode = [k for k in paged_kernels.values() if "fa_paged_decode_kernel<" in k.name]
    assert len(decode) == 8 * len(reachable) and len(paged_kernels) == len(decode) + 2, sorted(k.name for k in paged_kernels.values())
    # LDS: the two V images per wave and the merge, exactly what the contiguous-cache kernel of the same d takes
    kv = codeobj.kernels_of(_cabi_kv.LIB_PATH, str(tmp_path))
    kv_lds = {re.search(r"<(\d+),", k.name).group(1): k.lds for k in kv.values() if "fa_kv_decode_kernel<" in k.name}
    assert set(kv_lds) == {"64", "128"}
    for k in decode:
        assert k.lds == kv_lds[re.search(r"<(\d+),", k.name).group(1)], (k.name, k.lds, kv_lds)
