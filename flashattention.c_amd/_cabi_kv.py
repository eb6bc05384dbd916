"""ctypes view of include/flashattn_amd_kv.h (the KV-cache attention extension, libflashattn_amd_kv.so; this file only binds it)."""
from __future__ import annotations

from ._cabi import FA_DTYPE_BF16, FA_DTYPE_BF16_OUT_F32, FA_DTYPE_F32, FA_OK, ExtensionMissing, FlashAttnError  # noqa: F401
from ._cabi_ext import SHAPE, Extension, c_int, forward_args, i32, i64, queries, vp

# every symbol include/flashattn_amd_kv.h declares, in its order
_q = queries(SHAPE, SHAPE)
_ext = Extension("kv", _q[:2] + [("forward", forward_args(), c_int), ("stream_read", [vp, vp, i64, i64, i64, i32, vp, vp], c_int)] + _q[2:])
LIB_PATH, EXPORTED_SYMBOLS, bind, lib, check = _ext.LIB_PATH, _ext.EXPORTED_SYMBOLS, _ext.bind, _ext.lib, _ext.check
