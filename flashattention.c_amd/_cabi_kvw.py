"""ctypes view of include/flashattn_amd_kvw.h (sliding-window KV-cache attention, libflashattn_amd_kvw.so; this file only binds it)."""
from __future__ import annotations

from ._cabi import FA_DTYPE_BF16, FA_DTYPE_BF16_OUT_F32, FA_DTYPE_F32, FA_OK, ExtensionMissing, FlashAttnError  # noqa: F401
from ._cabi_ext import PAGED_SHAPE, SHAPE, WINDOW, Extension, FaPagedCache, c_int, forward_args, queries  # noqa: F401

# every symbol include/flashattn_amd_kvw.h declares, in its order
_ext = Extension("kvw", queries(SHAPE + WINDOW, SHAPE + WINDOW) + [("forward", forward_args(window=True), c_int)] +
                 queries(PAGED_SHAPE + WINDOW, None, "paged_") + [("paged_forward", forward_args(paged=True, window=True), c_int)])
LIB_PATH, EXPORTED_SYMBOLS, bind, lib, check = _ext.LIB_PATH, _ext.EXPORTED_SYMBOLS, _ext.bind, _ext.lib, _ext.check
