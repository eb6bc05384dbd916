"""CPU: the host side of the KV-cache attention extension (include/flashattn_amd_kv.h, libflashattn_amd_kv.so): the reference the GPU tests
use, the binding, argument validation (no device is touched before it passes), the plan, and the code objects of both libraries."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from flashattention_c_amd import _cabi, _cabi_kv
from oracle import oracle as orc
from tests import codeobj
from tests.conftest import GOLDEN_DIR
from tests.kv_reference import attention_kv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, 1, 2
BF16, BF16_F32, F32 = _cabi_kv.FA_DTYPE_BF16, _cabi_kv.FA_DTYPE_BF16_OUT_F32, _cabi_kv.FA_DTYPE_F32


@pytest.mark.parametrize("bh,nq,nk,d", [(3, 5, 37, 64), (2, 1, 130, 128)])
@pytest.mark.parametrize("causal", [False, True])
def test_the_reference_is_the_committed_oracle_on_the_padded_square_problem(bh, nq, nk, d, causal):
    rng = np.random.default_rng(nk)
    # fp32-representable values: the oracle takes fp32 tensors (and computes in fp64)
    q, k, v = (rng.standard_normal(s, dtype=np.float32).astype(np.float64) for s in ((bh, nq, d), (bh, nk, d), (bh, nk, d)))
    qp = np.zeros((bh, nk, d))
    qp[:, nk - nq:] = q
    o_sq, lse_sq = orc.attention_f64(qp, k, v, causal=causal, scale=0.3, return_lse=True)
    o, lse = attention_kv(q, k, v, None, causal, 0.3)
    assert np.abs(o - o_sq[:, nk - nq:]).max() < 1e-12 and np.abs(lse - lse_sq[:, nk - nq:]).max() < 1e-12


def test_reference_groups_lengths_and_rows_without_keys():
    rng = np.random.default_rng(1)
    q, k, v = rng.standard_normal((4, 3, 8)), rng.standard_normal((2, 6, 8)), rng.standard_normal((2, 6, 8))
    o, lse = attention_kv(q, k, v, [0, 2], True, 1.0)
    assert not o[:2].any() and np.all(lse[:2] == -np.inf)              # len 0
    assert not o[2:, 0].any() and np.all(lse[2:, 0] == -np.inf)          # len 2 < nq 3: row 0 sees nothing
    o1, _ = attention_kv(q[3:4], k[1:2, :2], v[1:2, :2], None, True, 1.0)  # query slab 3 reads K/V slab 1
    assert np.abs(o[3:4] - o1).max() < 1e-15


def test_header_prototypes_match_the_binding():
    hdr = open(os.path.join(ROOT, "include", "flashattn_amd_kv.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(fa_kv_[a-z_]+)\s*\(", hdr))
    assert declared == set(_cabi_kv.EXPORTED_SYMBOLS), declared ^ set(_cabi_kv.EXPORTED_SYMBOLS)
    L = _cabi_kv.lib()
    for sym in declared:
        assert getattr(L, sym) is not None
    assert b"gfx950" in L.fa_kv_version()
    import flashattention_c_amd as fa
    assert "forward_kv" in fa.__all__ and "workspace_bytes_kv" in fa.__all__ and callable(fa.forward_kv)


A = 0x7f0000000000   # pointers that are never dereferenced: validation comes before any device call


def _fwd(L, q=A, k=A + (1 << 30), v=A + (2 << 30), o=A + (3 << 30), lse=None, bh_kv=2, group=4, nq=1, nk=4096, cap=4096, lens=None, d=128, scale=1.0,
         causal=0, dtype=BF16, ws=None, ws_bytes=0):
    return L.fa_kv_forward(q, k, v, o, lse, bh_kv, group, nq, nk, cap, lens, d, scale, causal, dtype, ws, ws_bytes, None)


def test_validation_without_a_device():
    L = _cabi_kv.lib()
    need = L.fa_kv_workspace_bytes(2, 4, 1, 4096, 128, 0, BF16)
    assert need > 0
    cases = [
        (dict(q=None), INVALID), (dict(k=None), INVALID), (dict(v=None), INVALID), (dict(o=None), INVALID),
        (dict(q=A + 8), INVALID), (dict(ws=A + (5 << 30) + 128, ws_bytes=need), INVALID),
        (dict(nk=4097), INVALID),                                         # nk > capacity
        (dict(d=96), UNSUPPORTED), (dict(dtype=F32), UNSUPPORTED),
        (dict(scale=0.0), INVALID), (dict(scale=float("nan")), INVALID),
        (dict(nk=100, cap=4096, o=A + (1 << 30) + 4000 * 256), INVALID),     # o inside k's capacity range, beyond its first nk rows
        (dict(ws=A + (5 << 30), ws_bytes=need - 1), INVALID),                # workspace too small
        (dict(ws=A + (3 << 30), ws_bytes=need), INVALID),                    # workspace over o
        (dict(cap=1 << 24), UNSUPPORTED),                                    # 2^24 * 128 * 2 = 2^32 bytes per slab
        (dict(nk=(1 << 24) + 1, cap=(1 << 24) + 1, d=64), UNSUPPORTED),
        (dict(group=0), INVALID), (dict(nq=0), INVALID),
    ]
    for kw, code in cases:
        rc = _fwd(L, **kw)
        assert rc == code, (kw, rc, L.fa_kv_last_error())
        assert L.fa_kv_last_error(), kw
    assert _fwd(L, d=96) == UNSUPPORTED and b"64" in L.fa_kv_last_error() and b"128" in L.fa_kv_last_error()
    for args in ((2, 4, 1, 4096, 96, 0, BF16), (2, 4, 1, 4096, 128, 0, F32), (0, 4, 1, 4096, 128, 0, BF16), (2, 4, 1, (1 << 24) + 1, 128, 0, BF16)):
        assert L.fa_kv_workspace_bytes(*args) == 0 and L.fa_kv_splits_for(*args) == 0 and L.fa_kv_kernel_name_for(*args) is None
    assert L.fa_kv_stream_read(None, A, 2, 4096, 4096, 128, A + (4 << 30), None) == INVALID and L.fa_kv_last_error()


GRID = list(itertools.product((1, 2, 8, 64, 1024), (1, 4, 8), (1, 5, 16, 33), (1, 31, 256, 257, 4099, 32768, 1 << 24), (64, 128)))


def test_plan_properties_over_the_grid():
    L = _cabi_kv.lib()
    last = {}
    for bh_kv, group, nq, nk, d in GRID:
        S = L.fa_kv_splits_for(bh_kv, group, nq, nk, d, 0, BF16)
        ws = L.fa_kv_workspace_bytes(bh_kv, group, nq, nk, d, 0, BF16)
        what = (bh_kv, group, nq, nk, d, S, ws)
        assert 1 <= S <= 64, what
        assert S == L.fa_kv_splits_for(bh_kv, group, nq, nk, d, 1, BF16_F32), what
        if nk < 512:
            assert S == 1, what
        share = (-(-nk // S) + 63) // 64 * 64                     # ceil(nk / S) rounded up to 64 keys: a multiple of 64 by construction ...
        assert share % 64 == 0 and (S - 1) * share < nk <= S * share, what   # ... and every share non-empty at full length
        assert (ws == 0) == (S == 1), what
        if S > 1:
            assert ws >= S * bh_kv * group * nq * (d + 1) * 4, what
        key = (group, nq, nk, d)
        assert S <= last.get(key, 64), what                      # non-increasing in bh_kv (the grid walks bh_kv upwards)
        last[key] = S
    assert L.fa_kv_splits_for(1, 8, 1, 8192, 128, 0, BF16) >= 16


@pytest.fixture(scope="module")
def kv_kernels(tmp_path_factory):
    assert os.path.exists(_cabi_kv.LIB_PATH), "build the library first (python flashattention.c_amd/build.py)"
    return codeobj.kernels_of(_cabi_kv.LIB_PATH, str(tmp_path_factory.mktemp("co_kv")))


def _family(name: str) -> str:
    return re.sub(r"^void ", "", name).split("<")[0].split("(")[0].split("::")[-1]


def test_code_objects_of_the_kv_library(kv_kernels):
    spilling = [f"{k.scratch} B: {k.name}" for k in kv_kernels.values() if k.scratch != 0]
    assert not spilling, "\n".join(spilling)
    L = _cabi_kv.lib()
    reachable = set()
    for bh_kv, group, nq, nk, d in GRID:
        for causal, dt in ((0, BF16), (1, BF16_F32)):
            reachable.add(L.fa_kv_kernel_name_for(bh_kv, group, nq, nk, d, causal, dt).decode())
    helpers = {"fa_kv_combine_kernel", "fa_kv_stream_read_kernel"}
    present = {_family(k.name) for k in kv_kernels.values()}
    assert present == reachable | helpers, present ^ (reachable | helpers)
    # every instantiation the launcher can pick: d x causal x output type
    decode = [k.name for k in kv_kernels.values() if "fa_kv_decode_kernel<" in k.name]
    assert len(decode) == 8 and len(kv_kernels) == 11, sorted(k.name for k in kv_kernels.values())


def _sections(lib):
    out = subprocess.run([os.path.join(codeobj.LLVM_BIN, "llvm-readelf"), "-S", "-W", lib], capture_output=True, text=True, check=True).stdout
    return {n: int(sz, 16) for n, sz in re.findall(r"\]\s+(\.\S+)\s+\S+\s+[0-9a-f]+\s+[0-9a-f]+\s+([0-9a-f]+)", out)}


def test_the_product_library_is_what_the_parent_commit_builds(tmp_path):
    """ABI 6 is frozen and the headline kernels must not move: the extension adds a library, the product library keeps what a build of the
    commit before the extension gives it (tests/golden/kv_parent_kernels.txt): its kernel set, the size of every section that holds code or
    data -- .hip_fatbin (all device code), .text, .rodata, the relocation, symbol and unwind tables, ... to the byte -- and its file size.
    The file size of ONE source tree is not one number: hipcc names a symbol per translation unit `__hip_cuid_<hash of the source's path>`,
    hex WITHOUT leading zeros (1 .. 16 digits), and each name sits in .dynstr and in .strtab, so the same commit built in two directories
    differs by a few bytes there (observed: 4251544 and 4251552), and in the padding behind them.  Those two string tables and the padding
    section are therefore held to the most they can move: 15 characters per name and table, plus 8 bytes of alignment behind each table."""
    lines = open(os.path.join(GOLDEN_DIR, "kv_parent_kernels.txt")).read().splitlines()
    size = int(next(ln for ln in lines if ln.startswith("# size_bytes")).split()[-1])
    want = {ln.split()[2]: int(ln.split()[3], 16) for ln in lines if ln.startswith("# section")}
    names = {ln for ln in lines if ln and not ln.startswith("#")}
    assert set(codeobj.kernels_of(_cabi.LIB_PATH, str(tmp_path))) == names
    assert not any("fa_kv" in n for n in names)
    have = _sections(_cabi.LIB_PATH)
    free = {".dynstr", ".strtab", ".relro_padding"}
    assert set(have) - free == set(want) - free
    assert {n: have[n] for n in want if n not in free} == {n: want[n] for n in want if n not in free}
    units = subprocess.run([os.path.join(codeobj.LLVM_BIN, "llvm-readelf"), "--dyn-syms", "-W", _cabi.LIB_PATH], capture_output=True, text=True, check=True).stdout.count("__hip_cuid_")
    assert 20 <= units <= 40
    slack = 2 * (15 * units + 8)
    print(f"file size {os.path.getsize(_cabi.LIB_PATH)}, parent build {size}, {units} translation units: slack {slack} bytes")
    assert abs(os.path.getsize(_cabi.LIB_PATH) - size) <= slack
