"""CPU: the sliding-window chunked-prefill library (include/flashattn_amd_kvpw.h, libflashattn_amd_kvpw.so) without a device: its kernels and
their code-object properties (no scratch, the LDS of the unwindowed kernel, one wave per SIMD), its exports against the binding, the refusals
of its validator through ctypes (no call reaches a launch, no pointer is dereferenced) and the front end's keyword."""
import ctypes
import inspect
import os
import re

import pytest

import flashattention_c_amd as fa
from flashattention_c_amd import _cabi_kvpw
from tests import codeobj

BF16, BF16_F32, F32 = _cabi_kvpw.FA_DTYPE_BF16, _cabi_kvpw.FA_DTYPE_BF16_OUT_F32, _cabi_kvpw.FA_DTYPE_F32
INVALID, UNSUPPORTED = 1, 2
A, G = 0x7f0000000000, 1 << 30   # pointers that are never dereferenced: validation comes before any device call
Q, K, V, O, TABLE = A, A + 1 * G, A + 5 * G, A + 9 * G, A + 10 * G
LDS = {"fa_kvpw_prefill_kernel": 65536, "fa_kvpw8_prefill_kernel": 65536, "fa_kvpw256_prefill_kernel": 131072}


def forward(paged=False, fp8=False, **kw):
    a = dict(q=Q, B=2, H=2, group=4, nq=512, nk=4096, d=128, dtype=BF16, w=100, k_scale=1.0)
    assert set(kw) <= set(a)
    a.update(kw)
    L, scales = _cabi_kvpw.lib(), ((a["k_scale"], 1.0) if fp8 else ())
    tail = (a["d"], 1.0, *scales, 1, a["dtype"], a["w"], None)
    if paged:
        e = 1 if fp8 else 2
        cache = _cabi_kvpw.FaPagedCache(k_pool=K, v_pool=V, num_pages=256, page_size=64, page_stride=64 * 2 * a["d"], row_stride=2 * a["d"],
                                        head_stride=a["d"], block_table=TABLE, max_pages=64, seq_lens=None)
        assert e * cache.page_stride * 256 <= 4 * G
        rc = getattr(L, "fa_kvpw_fp8_paged_forward" if fp8 else "fa_kvpw_paged_forward")(a["q"], ctypes.byref(cache), O, None, a["B"], a["H"], a["group"], a["nq"], a["nk"], *tail)
    else:
        rc = getattr(L, "fa_kvpw_fp8_forward" if fp8 else "fa_kvpw_forward")(a["q"], K, V, O, None, a["B"], a["group"], a["nq"], a["nk"], a["nk"], None, *tail)
    return rc, L.fa_kvpw_last_error().decode()


REJECTED = [
    (False, False, dict(w=-1), INVALID, "window_left = -1 must be >= 0"),
    (True, False, dict(w=-5), INVALID, "window_left = -5 must be >= 0"),
    (False, True, dict(w=-1), INVALID, "window_left = -1 must be >= 0"),
    (True, True, dict(w=-(1 << 31)), INVALID, "must be >= 0"),
    (False, False, dict(d=64), UNSUPPORTED, "head dim 64 is not supported: 128 or 256"),
    (True, False, dict(d=96), UNSUPPORTED, "head dim 96 is not supported: 128 or 256"),
    (False, True, dict(d=256), UNSUPPORTED, "head dim 256 is not supported: 128"),
    (True, True, dict(d=256), UNSUPPORTED, "head dim 256 is not supported: 128"),
    (False, True, dict(k_scale=0.0), INVALID, "k_scale must be finite and > 0"),
    (False, False, dict(dtype=F32), UNSUPPORTED, "FA_DTYPE_F32 is not supported: caches are 16-bit"),
    (False, False, dict(q=Q + 8), INVALID, "q, k, v, o must be 16-byte aligned"),
]


@pytest.mark.parametrize("paged,fp8,kw,code,words", REJECTED, ids=[f"{'paged' if r[0] else 'contiguous'}-{'fp8' if r[1] else 'bf16'}-{r[2]}" for r in REJECTED])
def test_rejected_calls_reach_their_code_and_text(paged, fp8, kw, code, words):
    rc, text = forward(paged, fp8, **kw)
    assert rc == code and words in text, (rc, text)


def test_kernel_name_by_head_dim_and_the_front_end_keyword():
    L = _cabi_kvpw.lib()
    for dt in (BF16, BF16_F32):
        for w in (0, 4095, 1 << 24, 0x7fffffff):   # wider than 2^24 saturates
            assert L.fa_kvpw_kernel_name_for(8, 4, 2048, 32768, 128, 1, dt, w) == b"fa_kvpw_prefill_kernel"
            assert L.fa_kvpw_kernel_name_for(2, 8, 70, 321, 256, 0, dt, w) == b"fa_kvpw256_prefill_kernel"
    for args in [(2, 4, 512, 4096, 64, 1, BF16, 5), (2, 4, 512, 4096, 128, 1, F32, 5), (2, 4, 512, 4096, 128, 1, BF16, -1), (0, 4, 512, 4096, 256, 1, BF16, 5)]:
        assert L.fa_kvpw_kernel_name_for(*args) is None, args
    for name in ("prefill_kv", "prefill_paged", "prefill_kv_fp8", "prefill_paged_fp8"):
        assert inspect.signature(getattr(fa, name)).parameters["window_left"].default is None
    with pytest.raises(ValueError, match="window_left = -1 must be >= 0"):   # checked first: before the tensors are looked at
        fa.prefill_kv(None, None, None, window_left=-1)
    with pytest.raises(TypeError, match="window_left must be None or an int"):
        fa.prefill_paged_fp8(None, None, None, None, window_left=1.5)


def test_code_objects_have_no_scratch_the_unwindowed_lds_one_wave_per_simd_and_the_exports_of_the_binding(tmp_path):
    ks = codeobj.kernels_of(_cabi_kvpw.LIB_PATH, str(tmp_path))
    fams = sorted(k.name.split("<")[0].split("::")[-1].split()[-1] for k in ks.values())
    assert fams == sorted(8 * list(LDS)), fams   # paged x causal x fp32 output of each loop / dtype
    for k in ks.values():
        print(f"{k.name}: lds {k.lds} scratch {k.scratch} regs {k.vgprs} + {k.agprs}")
        assert k.scratch == 0 and k.lds == LDS[k.name.split("<")[0].split("::")[-1].split()[-1]], k.name
        assert k.vgprs > 256, k.name   # (the total of both halves) more than half of a SIMD's 512 registers: one wave per SIMD
    names = set(re.findall(r" T (fa_\w+)", os.popen(f"nm -D --defined-only {_cabi_kvpw.LIB_PATH}").read()))
    assert names == set(_cabi_kvpw.EXPORTED_SYMBOLS), names ^ set(_cabi_kvpw.EXPORTED_SYMBOLS)
