"""ctypes view of include/flashattn_amd_kvpw.h (chunked prefill under a sliding window: bf16 caches at head dims 128 and 256, fp8 at 128,
libflashattn_amd_kvpw.so; this file only binds it)."""
from __future__ import annotations

from ._cabi import FA_DTYPE_BF16, FA_DTYPE_BF16_OUT_F32, FA_DTYPE_F32, FA_OK, ExtensionMissing, FlashAttnError  # noqa: F401
from ._cabi_ext import SHAPE, WINDOW, Extension, FaPagedCache, c_int, c_str, forward_args  # noqa: F401
from ._cabi_kvp import _without_workspace

# every symbol include/flashattn_amd_kvpw.h declares, in its order
_ext = Extension("kvpw", [("kernel_name_for", SHAPE + WINDOW, c_str), ("forward", _without_workspace(forward_args(window=True)), c_int),
                          ("paged_forward", _without_workspace(forward_args(paged=True, window=True)), c_int),
                          ("fp8_forward", _without_workspace(forward_args(fp8=True, window=True)), c_int),
                          ("fp8_paged_forward", _without_workspace(forward_args(paged=True, fp8=True, window=True)), c_int)])
LIB_PATH, EXPORTED_SYMBOLS, bind, lib, check = _ext.LIB_PATH, _ext.EXPORTED_SYMBOLS, _ext.bind, _ext.lib, _ext.check
