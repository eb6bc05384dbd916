"""CPU: the fp8 chunked-prefill library (include/flashattn_amd_kvp8.h, libflashattn_amd_kvp8.so) without a device: every rejected call through
ctypes reaches the code and the text the fp8 decode library gives for the same fault (no call reaches a launch, no pointer is dereferenced),
the kernel-name query, and the code object: no scratch, the LDS of one CU, the exports of the binding."""
import ctypes
import os
import re

import pytest

import flashattention_c_amd as fa
from flashattention_c_amd import _cabi_kvp8, flash
from tests import codeobj

BF16, BF16_F32, F32 = _cabi_kvp8.FA_DTYPE_BF16, _cabi_kvp8.FA_DTYPE_BF16_OUT_F32, _cabi_kvp8.FA_DTYPE_F32
INVALID, UNSUPPORTED = 1, 2
A, G = 0x7f0000000000, 1 << 30   # pointers that are never dereferenced: validation comes before any device call
Q, K, V, O, TABLE = A, A + 1 * G, A + 5 * G, A + 9 * G, A + 10 * G


def forward(paged=False, **kw):
    a = dict(q=Q, o=O, B=2, H=2, group=4, nq=512, nk=4096, cap=4096, d=128, dtype=BF16, page_size=64, row_stride=2 * 128, k_scale=0.5, v_scale=2.0)
    assert set(kw) <= set(a)
    a.update(kw)
    L = _cabi_kvp8.lib()
    if paged:
        cache = _cabi_kvp8.FaPagedCache(k_pool=K, v_pool=V, num_pages=256, page_size=a["page_size"], page_stride=64 * 2 * 128, row_stride=a["row_stride"],
                                        head_stride=128, block_table=TABLE, max_pages=64, seq_lens=None)
        rc = L.fa_kvp8_paged_forward(a["q"], ctypes.byref(cache), a["o"], None, a["B"], a["H"], a["group"], a["nq"], a["nk"], a["d"], 1.0, a["k_scale"],
                                     a["v_scale"], 1, a["dtype"], None)
    else:
        rc = L.fa_kvp8_forward(a["q"], K, V, a["o"], None, a["B"], a["group"], a["nq"], a["nk"], a["cap"], None, a["d"], 1.0, a["k_scale"], a["v_scale"], 1,
                               a["dtype"], None)
    return rc, L.fa_kvp8_last_error().decode()


REJECTED = [
    (False, dict(d=64), UNSUPPORTED, "head dim 64 is not supported: 128"),
    (True, dict(d=256), UNSUPPORTED, "head dim 256 is not supported: 128"),
    (False, dict(dtype=F32), UNSUPPORTED, "FA_DTYPE_F32 is not supported: q and o are as in fa_kv_forward"),
    (False, dict(k_scale=-1.0), INVALID, "k_scale must be finite and > 0"),
    (True, dict(v_scale=float("inf")), INVALID, "v_scale must be finite and > 0"),
    (False, dict(q=Q + 8), INVALID, "q, k8, v8, o must be 16-byte aligned"),
    (False, dict(o=K + 4096), INVALID, "o overlaps q, k8 or v8"),
    (False, dict(cap=1 << 25), UNSUPPORTED, "a K/V slab (capacity * d bytes) must stay below 2^32 bytes"),
    (True, dict(page_size=24), UNSUPPORTED, "page_size 24 is not supported"),
    (True, dict(row_stride=2 * 128 + 8), INVALID, "must be multiples of 16 elements (16 bytes)"),
]


@pytest.mark.parametrize("paged,kw,code,words", REJECTED, ids=[f"{'paged' if r[0] else 'contiguous'}-{r[1]}" for r in REJECTED])
def test_rejected_calls_reach_their_code_and_text(paged, kw, code, words):
    rc, text = forward(paged, **kw)
    assert rc == code and words in text, (rc, text)


def test_kernel_name_exactly_for_accepted_shapes_and_the_front_end_exports():
    L = _cabi_kvp8.lib()
    for dt in (BF16, BF16_F32):
        for shape in ((1, 1, 1, 1), (8, 4, 2048, 32768), (2, 8, 70, 321)):
            assert L.fa_kvp8_kernel_name_for(*shape, 128, 1, dt) == b"fa_kvp8_prefill_kernel"
    for args in [(2, 4, 512, 4096, 64, 1, BF16), (2, 4, 512, 4096, 256, 0, BF16), (2, 4, 512, 4096, 128, 1, F32), (0, 4, 512, 4096, 128, 1, BF16),
                 (2, 4, 512, (1 << 24) + 1, 128, 1, BF16)]:
        assert L.fa_kvp8_kernel_name_for(*args) is None, args
    for name in ("prefill_kv_fp8", "prefill_paged_fp8"):
        assert name in fa.__all__ and name in flash.__all__ and callable(getattr(fa, name))


def test_code_object_has_no_scratch_fits_a_cu_and_exports_the_binding(tmp_path):
    ks = codeobj.kernels_of(_cabi_kvp8.LIB_PATH, str(tmp_path))
    assert len(ks) == 8 and all("fa_kvp8_prefill_kernel<" in k.name for k in ks.values()), sorted(k.name for k in ks.values())
    for k in ks.values():   # paged x causal x fp32 output
        print(f"{k.name}: lds {k.lds} scratch {k.scratch} regs {k.vgprs} + {k.agprs}")
        assert k.scratch == 0 and k.lds <= 160 * 1024, k.name
    names = set(re.findall(r" T (fa_\w+)", os.popen(f"nm -D --defined-only {_cabi_kvp8.LIB_PATH}").read()))
    assert names == set(_cabi_kvp8.EXPORTED_SYMBOLS), names ^ set(_cabi_kvp8.EXPORTED_SYMBOLS)
