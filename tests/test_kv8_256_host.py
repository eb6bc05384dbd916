"""CPU: the head-dim-256 fp8 KV-cache library (include/flashattn_amd_kv8_256.h, libflashattn_amd_kv8_256.so) without a device: every rejected
call through ctypes (no call reaches a launch, no pointer is dereferenced), the queries against those of the bf16 library at d = 256, and
the code object: sixteen decode kernels, no scratch, the LDS of one CU, the exports of the binding."""
import ctypes
import os
import re

import pytest

from flashattention_c_amd import _cabi_kv8_256, _cabi_kv256
from tests import codeobj

BF16, BF16_F32, F32 = _cabi_kv8_256.FA_DTYPE_BF16, _cabi_kv8_256.FA_DTYPE_BF16_OUT_F32, _cabi_kv8_256.FA_DTYPE_F32
INVALID, UNSUPPORTED = 1, 2
A, G = 0x7f0000000000, 1 << 30   # pointers that are never dereferenced: validation comes before any device call
Q, K, V, O, WS, TABLE = A, A + 1 * G, A + 2 * G, A + 3 * G, A + 5 * G, A + 6 * G
INF = float("inf")


def forward(paged=False, **kw):
    a = dict(q=Q, o=O, B=2, H=2, group=4, nq=1, nk=4096, cap=4096, d=256, dtype=BF16, window=-1, ws=None, ws_bytes=0, page_size=64, row_stride=2 * 256,
             scale=1.0, k_scale=0.013, v_scale=0.011)
    assert set(kw) <= set(a)
    a.update(kw)
    L = _cabi_kv8_256.lib()
    if paged:
        cache = _cabi_kv8_256.FaPagedCache(k_pool=K, v_pool=V, num_pages=256, page_size=a["page_size"], page_stride=64 * 2 * 256, row_stride=a["row_stride"],
                                           head_stride=256, block_table=TABLE, max_pages=64, seq_lens=None)
        rc = L.fa_kv8_256_paged_forward(a["q"], ctypes.byref(cache), a["o"], None, a["B"], a["H"], a["group"], a["nq"], a["nk"], a["d"], a["scale"],
                                        a["k_scale"], a["v_scale"], 1, a["dtype"], a["window"], a["ws"], a["ws_bytes"], None)
    else:
        rc = L.fa_kv8_256_forward(a["q"], K, V, a["o"], None, a["B"], a["group"], a["nq"], a["nk"], a["cap"], None, a["d"], a["scale"], a["k_scale"],
                                  a["v_scale"], 1, a["dtype"], a["window"], a["ws"], a["ws_bytes"], None)
    return rc, L.fa_kv8_256_last_error().decode()


NEED = _cabi_kv256.lib().fa_kv256_workspace_bytes(2, 4, 1, 4096, 256, 1, BF16, -1)
REJECTED = [
    (False, dict(d=64), UNSUPPORTED, "head dim 64 is not supported: 256"),
    (False, dict(d=128), UNSUPPORTED, "head dim 128 is not supported: 256"),
    (True, dict(d=96), UNSUPPORTED, "head dim 96 is not supported: 256"),
    (False, dict(dtype=F32), UNSUPPORTED, "FA_DTYPE_F32 is not supported: q and o are as in fa_kv_forward"),
    (False, dict(window=-2), INVALID, "window_left = -2 must be >= 0, or -1 for no window"),
    (True, dict(window=-2), INVALID, "window_left = -2"),
    (False, dict(k_scale=0.0), INVALID, "k_scale must be finite and > 0"),
    (True, dict(k_scale=INF), INVALID, "k_scale must be finite and > 0"),
    (False, dict(v_scale=-1.0), INVALID, "v_scale must be finite and > 0"),
    (True, dict(v_scale=INF), INVALID, "v_scale must be finite and > 0"),
    (False, dict(scale=INF), INVALID, "scale must be finite and non-zero"),
    (False, dict(cap=1 << 24), UNSUPPORTED, "a K/V slab (capacity * d bytes) must stay below 2^32 bytes"),
    (False, dict(ws=WS, ws_bytes=NEED - 1), INVALID, f"is too small: fa_kv8_256_workspace_bytes() = {NEED}"),
    (True, dict(B=1, ws=WS, ws_bytes=NEED - 1), INVALID, f"is too small: fa_kv8_256_paged_workspace_bytes() = {NEED}"),
    (True, dict(row_stride=2 * 256 + 8), INVALID, "must be multiples of 16 elements (16 bytes)"),
]


@pytest.mark.parametrize("paged,kw,code,words", REJECTED, ids=[f"{'paged' if r[0] else 'contiguous'}-{r[1]}" for r in REJECTED])
def test_rejected_calls_reach_their_code_and_text(paged, kw, code, words):
    assert NEED > 0
    rc, text = forward(paged, **kw)
    assert rc == code and words in text, (rc, text)


def test_queries_equal_those_of_the_bf16_library_at_d_256():
    L, R = _cabi_kv8_256.lib(), _cabi_kv256.lib()
    for bh in (1, 2, 8, 64, 300):
        for g, nq in ((1, 1), (8, 1), (4, 5), (4, 33)):
            for nk in (1, 255, 512, 1000, 4099, 65536):
                for w in (-1, 0, 100, 4095):
                    for dt in (BF16, BF16_F32):
                        a, p = (bh, g, nq, nk, 256, 1, dt, w), (bh, 2, g, nq, nk, 256, 1, dt, w)
                        assert L.fa_kv8_256_splits_for(*a) == R.fa_kv256_splits_for(*a) >= 1, a
                        assert L.fa_kv8_256_workspace_bytes(*a) == R.fa_kv256_workspace_bytes(*a), a
                        assert L.fa_kv8_256_paged_splits_for(*p) == R.fa_kv256_paged_splits_for(*p) >= 1, p
                        assert L.fa_kv8_256_paged_workspace_bytes(*p) == R.fa_kv256_paged_workspace_bytes(*p), p
    for args in [(2, 4, 1, 4096, 128, 1, BF16, -1), (2, 4, 1, 4096, 256, 1, F32, -1), (2, 4, 1, 4096, 256, 1, BF16, -2), (0, 4, 1, 4096, 256, 1, BF16, 5)]:
        assert L.fa_kv8_256_workspace_bytes(*args) == 0 and L.fa_kv8_256_splits_for(*args) == 0 and L.fa_kv8_256_kernel_name_for(*args) is None
    assert L.fa_kv8_256_kernel_name_for(2, 4, 1, 4096, 256, 1, BF16, -1) == b"fa_kv8_256_decode_kernel"


def test_code_object_has_no_scratch_fits_a_cu_and_exports_the_binding(tmp_path):
    ks = codeobj.kernels_of(_cabi_kv8_256.LIB_PATH, str(tmp_path))
    decode = [k for k in ks.values() if "fa_kv8_256_decode_kernel<" in k.name]
    assert len(decode) == 16 and len(ks) == 16 + sum(1 for k in ks.values() if "combine" in k.name), sorted(k.name for k in ks.values())
    for k in decode:   # paged x window x causal x fp32 output
        print(f"{k.name}: lds {k.lds} scratch {k.scratch} regs {k.vgprs} + {k.agprs}")
        assert k.scratch == 0 and k.lds <= 160 * 1024, k.name
    names = set(re.findall(r" T (fa_\w+)", os.popen(f"nm -D --defined-only {_cabi_kv8_256.LIB_PATH}").read()))
    assert names == set(_cabi_kv8_256.EXPORTED_SYMBOLS), names ^ set(_cabi_kv8_256.EXPORTED_SYMBOLS)
