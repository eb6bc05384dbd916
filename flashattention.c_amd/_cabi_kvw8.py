"""ctypes view of include/flashattn_amd_kvw8.h (sliding-window KV-cache attention over an fp8 e4m3fn cache, libflashattn_amd_kvw8.so; this file only binds it)."""
from __future__ import annotations

from ._cabi import FA_DTYPE_BF16, FA_DTYPE_BF16_OUT_F32, FA_DTYPE_F32, FA_OK, ExtensionMissing, FlashAttnError  # noqa: F401
from ._cabi_ext import PAGE_SIZE, PAGED_SHAPE, SHAPE, WINDOW, Extension, FaPagedCache, c_int, forward_args, queries  # noqa: F401

# every symbol include/flashattn_amd_kvw8.h declares, in its order
_ext = Extension("kvw8", queries(SHAPE + WINDOW, SHAPE + PAGE_SIZE + WINDOW) + [("forward", forward_args(fp8=True, window=True), c_int)] +
                 queries(PAGED_SHAPE + WINDOW, None, "paged_") + [("paged_forward", forward_args(paged=True, fp8=True, window=True), c_int)])
LIB_PATH, EXPORTED_SYMBOLS, bind, lib, check = _ext.LIB_PATH, _ext.EXPORTED_SYMBOLS, _ext.bind, _ext.lib, _ext.check
