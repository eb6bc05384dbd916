"""ctypes view of include/flashattn_amd_kv8.h (KV-cache attention over an fp8 e4m3fn cache, contiguous and paged: libflashattn_amd_kv8.so;
this file only binds it)."""
from __future__ import annotations

from ._cabi import FA_DTYPE_BF16, FA_DTYPE_BF16_OUT_F32, FA_DTYPE_F32, FA_OK, ExtensionMissing, FlashAttnError  # noqa: F401
from ._cabi_ext import PAGE_SIZE, SHAPE, Extension, FaPagedCache, c_int, forward_args, queries  # noqa: F401

# every symbol include/flashattn_amd_kv8.h declares, in its order
_ext = Extension("kv8", queries(SHAPE, SHAPE + PAGE_SIZE) + [("forward", forward_args(fp8=True), c_int), ("paged_forward", forward_args(paged=True, fp8=True), c_int)])
LIB_PATH, EXPORTED_SYMBOLS, bind, lib, check = _ext.LIB_PATH, _ext.EXPORTED_SYMBOLS, _ext.bind, _ext.lib, _ext.check
