"""CPU: the head-dim-256 KV-cache library (include/flashattn_amd_kv256.h, libflashattn_amd_kv256.so) without a device: every rejected call
through ctypes (no call reaches a launch, no pointer is dereferenced), the queries against the kv_plan formula of csrc/fa_kv.h, and the code
object: no scratch, the LDS of one CU, the exports of the binding."""
import ctypes
import os
import re

import pytest

from flashattention_c_amd import _cabi_kv256
from tests import codeobj

BF16, BF16_F32, F32 = _cabi_kv256.FA_DTYPE_BF16, _cabi_kv256.FA_DTYPE_BF16_OUT_F32, _cabi_kv256.FA_DTYPE_F32
INVALID, UNSUPPORTED = 1, 2
A, G = 0x7f0000000000, 1 << 30   # pointers that are never dereferenced: validation comes before any device call
Q, K, V, O, WS, TABLE = A, A + 1 * G, A + 2 * G, A + 3 * G, A + 5 * G, A + 6 * G


def plan(bh_kv, group, nq, nk, d=256):
    """kv_plan and kv_workspace_bytes of csrc/fa_kv.h: 256 target workgroups, no share below 256 keys, at most 64 shares of a multiple of 64 keys"""
    wgs = bh_kv * -(-group * nq // 32)
    s = max(1, min(-(-256 // wgs), nk // 256, 64))
    while True:
        share = (-(-nk // s) + 63) // 64 * 64
        if s > 1 and (s - 1) * share >= nk:
            s -= 1
        else:
            break
    return s, 0 if s == 1 else (s * bh_kv * group * nq * (d + 1) * 4 + 255) // 256 * 256


def forward(paged=False, **kw):
    a = dict(q=Q, o=O, B=2, H=2, group=4, nq=1, nk=4096, cap=4096, d=256, dtype=BF16, window=-1, ws=None, ws_bytes=0, page_size=64)
    assert set(kw) <= set(a)
    a.update(kw)
    L = _cabi_kv256.lib()
    if paged:
        cache = _cabi_kv256.FaPagedCache(k_pool=K, v_pool=V, num_pages=256, page_size=a["page_size"], page_stride=64 * 2 * 256, row_stride=2 * 256,
                                         head_stride=256, block_table=TABLE, max_pages=64, seq_lens=None)
        rc = L.fa_kv256_paged_forward(a["q"], ctypes.byref(cache), a["o"], None, a["B"], a["H"], a["group"], a["nq"], a["nk"], a["d"], 1.0, 1, a["dtype"],
                                      a["window"], a["ws"], a["ws_bytes"], None)
    else:
        rc = L.fa_kv256_forward(a["q"], K, V, a["o"], None, a["B"], a["group"], a["nq"], a["nk"], a["cap"], None, a["d"], 1.0, 1, a["dtype"], a["window"],
                                a["ws"], a["ws_bytes"], None)
    return rc, L.fa_kv256_last_error().decode()


NEED = plan(2, 4, 1, 4096)[1]
REJECTED = [
    (False, dict(d=64), UNSUPPORTED, "head dim 64 is not supported: 256"),
    (False, dict(d=128), UNSUPPORTED, "head dim 128 is not supported: 256"),
    (True, dict(d=96), UNSUPPORTED, "head dim 96 is not supported: 256"),
    (False, dict(dtype=F32), UNSUPPORTED, "FA_DTYPE_F32 is not supported: caches are 16-bit"),
    (False, dict(window=-2), INVALID, "window_left = -2 must be >= 0, or -1 for no window"),
    (True, dict(window=-2), INVALID, "window_left = -2"),
    (False, dict(cap=1 << 23), UNSUPPORTED, "must stay below 2^32 bytes"),
    (False, dict(ws=WS, ws_bytes=NEED - 1), INVALID, f"is too small: fa_kv256_workspace_bytes() = {NEED}"),
    (False, dict(q=Q + 8), INVALID, "q, k, v, o must be 16-byte aligned"),
    (True, dict(page_size=24), UNSUPPORTED, "page_size 24 is not supported"),
]


@pytest.mark.parametrize("paged,kw,code,words", REJECTED, ids=[f"{'paged' if r[0] else 'contiguous'}-{r[1]}" for r in REJECTED])
def test_rejected_calls_reach_their_code_and_text(paged, kw, code, words):
    assert NEED > 0
    rc, text = forward(paged, **kw)
    assert rc == code and words in text, (rc, text)


def test_queries_equal_the_plan_formula():
    L = _cabi_kv256.lib()
    for bh in (1, 2, 8, 64, 300):
        for g, nq in ((1, 1), (8, 1), (4, 5), (4, 33)):
            for nk in (1, 255, 512, 1000, 4099, 65536):
                S, ws = plan(bh, g, nq, nk)
                for dt in (BF16, BF16_F32):
                    assert L.fa_kv256_splits_for(bh, g, nq, nk, 256, 1, dt, -1) == S, (bh, g, nq, nk)
                    assert L.fa_kv256_workspace_bytes(bh, g, nq, nk, 256, 0, dt, -1) == ws
                    assert L.fa_kv256_paged_splits_for(bh, 2, g, nq, nk, 256, 1, dt, -1) == plan(2 * bh, g, nq, nk)[0]
                for w in (0, 100, 4095):   # under a window the plan is laid over span = min(nk, window_left + nq + 63)
                    Sw, wsw = plan(bh, g, nq, min(nk, w + nq + 63))
                    assert L.fa_kv256_splits_for(bh, g, nq, nk, 256, 1, BF16, w) == Sw
                    assert L.fa_kv256_paged_workspace_bytes(bh, 1, g, nq, nk, 256, 1, BF16, w) == wsw
    for args in [(2, 4, 1, 4096, 128, 1, BF16, -1), (2, 4, 1, 4096, 256, 1, F32, -1), (2, 4, 1, 4096, 256, 1, BF16, -2), (0, 4, 1, 4096, 256, 1, BF16, 5)]:
        assert L.fa_kv256_workspace_bytes(*args) == 0 and L.fa_kv256_splits_for(*args) == 0 and L.fa_kv256_kernel_name_for(*args) is None
    assert L.fa_kv256_kernel_name_for(2, 4, 1, 4096, 256, 1, BF16, -1) == b"fa_kv256_decode_kernel"


def test_code_object_has_no_scratch_fits_a_cu_and_exports_the_binding(tmp_path):
    ks = codeobj.kernels_of(_cabi_kv256.LIB_PATH, str(tmp_path))
    decode = [k for k in ks.values() if "fa_kv256_decode_kernel<" in k.name]
    assert len(decode) == 16 and len(ks) == 16 + sum(1 for k in ks.values() if "combine" in k.name), sorted(k.name for k in ks.values())
    for k in decode:   # paged x window x causal x fp32 output
        print(f"{k.name}: lds {k.lds} scratch {k.scratch} regs {k.vgprs} + {k.agprs}")
        assert k.scratch == 0 and k.lds <= 160 * 1024, k.name
    names = set(re.findall(r" T (fa_\w+)", os.popen(f"nm -D --defined-only {_cabi_kv256.LIB_PATH}").read()))
    assert names == set(_cabi_kv256.EXPORTED_SYMBOLS), names ^ set(_cabi_kv256.EXPORTED_SYMBOLS)
