"""ctypes view of include/flashattn_amd_kvp256.h (chunked prefill over the bf16 K/V caches at head dim 256, libflashattn_amd_kvp256.so; this file only binds it)."""
from __future__ import annotations

from ._cabi import FA_DTYPE_BF16, FA_DTYPE_BF16_OUT_F32, FA_DTYPE_F32, FA_OK, ExtensionMissing, FlashAttnError  # noqa: F401
from ._cabi_ext import SHAPE, Extension, FaPagedCache, c_int, c_str, forward_args  # noqa: F401
from ._cabi_kvp import _without_workspace

# every symbol include/flashattn_amd_kvp256.h declares, in its order
_ext = Extension("kvp256", [("kernel_name_for", SHAPE, c_str), ("forward", _without_workspace(forward_args()), c_int),
                            ("paged_forward", _without_workspace(forward_args(paged=True)), c_int)])
LIB_PATH, EXPORTED_SYMBOLS, bind, lib, check = _ext.LIB_PATH, _ext.EXPORTED_SYMBOLS, _ext.bind, _ext.lib, _ext.check
