"""CPU: the chunked-prefill library at head dim 256 (include/flashattn_amd_kvp256.h, libflashattn_amd_kvp256.so) without a device: every
rejected call through ctypes (no call reaches a launch, no pointer is dereferenced), the kernel-name query, the code object (no scratch, the
LDS of one CU, the exports of the binding) and the front end's choice of library by head dim."""
import ctypes
import os
import re

import pytest

from flashattention_c_amd import _cabi_kvp, _cabi_kvp8, _cabi_kvp256, flash
from tests import codeobj

BF16, BF16_F32, F32 = _cabi_kvp256.FA_DTYPE_BF16, _cabi_kvp256.FA_DTYPE_BF16_OUT_F32, _cabi_kvp256.FA_DTYPE_F32
INVALID, UNSUPPORTED = 1, 2
A, G = 0x7f0000000000, 1 << 30   # pointers that are never dereferenced: validation comes before any device call
Q, K, V, O, TABLE = A, A + 1 * G, A + 5 * G, A + 9 * G, A + 10 * G


def forward(paged=False, **kw):
    a = dict(q=Q, o=O, B=2, H=2, group=4, nq=512, nk=4096, cap=4096, d=256, dtype=BF16, page_size=64)
    assert set(kw) <= set(a)
    a.update(kw)
    L = _cabi_kvp256.lib()
    if paged:
        cache = _cabi_kvp256.FaPagedCache(k_pool=K, v_pool=V, num_pages=256, page_size=a["page_size"], page_stride=64 * 2 * 256, row_stride=2 * 256,
                                          head_stride=256, block_table=TABLE, max_pages=64, seq_lens=None)
        rc = L.fa_kvp256_paged_forward(a["q"], ctypes.byref(cache), a["o"], None, a["B"], a["H"], a["group"], a["nq"], a["nk"], a["d"], 1.0, 1, a["dtype"], None)
    else:
        rc = L.fa_kvp256_forward(a["q"], K, V, a["o"], None, a["B"], a["group"], a["nq"], a["nk"], a["cap"], None, a["d"], 1.0, 1, a["dtype"], None)
    return rc, L.fa_kvp256_last_error().decode()


REJECTED = [
    (False, dict(d=128), UNSUPPORTED, "head dim 128 is not supported: 256"),
    (True, dict(d=64), UNSUPPORTED, "head dim 64 is not supported: 256"),
    (False, dict(dtype=F32), UNSUPPORTED, "FA_DTYPE_F32 is not supported: caches are 16-bit"),
    (False, dict(q=Q + 8), INVALID, "q, k, v, o must be 16-byte aligned"),
    (False, dict(o=K + 4096), INVALID, "o overlaps q, k or v"),
    (False, dict(cap=1 << 23), UNSUPPORTED, "must stay below 2^32 bytes"),
    (True, dict(page_size=24), UNSUPPORTED, "page_size 24 is not supported"),
]


@pytest.mark.parametrize("paged,kw,code,words", REJECTED, ids=[f"{'paged' if r[0] else 'contiguous'}-{r[1]}" for r in REJECTED])
def test_rejected_calls_reach_their_code_and_text(paged, kw, code, words):
    rc, text = forward(paged, **kw)
    assert rc == code and words in text, (rc, text)


def test_kernel_name_exactly_for_accepted_shapes():
    L = _cabi_kvp256.lib()
    for dt in (BF16, BF16_F32):
        for shape in ((1, 1, 1, 1), (8, 4, 2048, 32768), (2, 8, 70, 321)):
            assert L.fa_kvp256_kernel_name_for(*shape, 256, 1, dt) == b"fa_kvp256_prefill_kernel"
    for args in [(2, 4, 512, 4096, 128, 1, BF16), (2, 4, 512, 4096, 256, 1, F32), (0, 4, 512, 4096, 256, 1, BF16)]:
        assert L.fa_kvp256_kernel_name_for(*args) is None, args


def test_code_object_has_no_scratch_fits_a_cu_and_exports_the_binding(tmp_path):
    ks = codeobj.kernels_of(_cabi_kvp256.LIB_PATH, str(tmp_path))
    assert len(ks) == 8 and all("fa_kvp256_prefill_kernel<" in k.name for k in ks.values()), sorted(k.name for k in ks.values())
    for k in ks.values():   # paged x causal x fp32 output
        print(f"{k.name}: lds {k.lds} scratch {k.scratch} regs {k.vgprs} + {k.agprs}")
        assert k.scratch == 0 and k.lds <= 160 * 1024, k.name
    names = set(re.findall(r" T (fa_\w+)", os.popen(f"nm -D --defined-only {_cabi_kvp256.LIB_PATH}").read()))
    assert names == set(_cabi_kvp256.EXPORTED_SYMBOLS), names ^ set(_cabi_kvp256.EXPORTED_SYMBOLS)


def test_the_front_end_picks_the_library_by_head_dim():
    for paged, tail in ((False, "forward"), (True, "paged_forward")):
        assert flash._prefill_entry("prefill_kv", 128, False, paged) == (_cabi_kvp, "fa_kvp_" + tail)
        assert flash._prefill_entry("prefill_kv", 256, False, paged) == (_cabi_kvp256, "fa_kvp256_" + tail)
        assert flash._prefill_entry("prefill_kv_fp8", 128, True, paged) == (_cabi_kvp8, "fa_kvp8_" + tail)
        with pytest.raises(ValueError, match="head_dim 256 not supported by prefill_kv_fp8"):
            flash._prefill_entry("prefill_kv_fp8", 256, True, paged)
        with pytest.raises(ValueError, match="head_dim 64 not supported by prefill_paged"):
            flash._prefill_entry("prefill_paged", 64, False, paged)
