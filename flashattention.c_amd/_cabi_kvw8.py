"""ctypes view of include/flashattn_amd_kvw8.h (sliding-window KV-cache attention over an fp8 e4m3fn cache, libflashattn_amd_kvw8.so; this file only binds it)."""
from __future__ import annotations

import ctypes
import os

from ._cabi import FA_DTYPE_BF16, FA_DTYPE_BF16_OUT_F32, FA_DTYPE_F32, FA_OK, ExtensionMissing, FlashAttnError  # noqa: F401
from ._cabi_paged import FaPagedCache  # noqa: F401  (the struct of include/flashattn_amd_paged.h, its pools read as e4m3 bytes)

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libflashattn_amd_kvw8.so")

# every symbol include/flashattn_amd_kvw8.h declares
EXPORTED_SYMBOLS = (
    "fa_kvw8_workspace_bytes", "fa_kvw8_splits_for", "fa_kvw8_kernel_name_for", "fa_kvw8_forward",
    "fa_kvw8_paged_workspace_bytes", "fa_kvw8_paged_splits_for", "fa_kvw8_paged_forward", "fa_kvw8_last_error", "fa_kvw8_version",
)

_libs = {}


def bind(path: str) -> ctypes.CDLL:
    """Load a build of the library and declare its prototypes."""
    L = ctypes.CDLL(path)
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    shape = [i64, i32, i64, i64, i32, i32, i32, i32]   # bh_kv, group, nq, nk, d, causal, dtype, window_left
    L.fa_kvw8_workspace_bytes.argtypes = shape
    L.fa_kvw8_workspace_bytes.restype = ctypes.c_size_t
    L.fa_kvw8_splits_for.argtypes = shape
    L.fa_kvw8_splits_for.restype = i32
    L.fa_kvw8_kernel_name_for.argtypes = shape[:-1] + [i32, i32]   # ..., dtype, page_size, window_left
    L.fa_kvw8_kernel_name_for.restype = ctypes.c_char_p
    L.fa_kvw8_forward.argtypes = [vp, vp, vp, vp, vp, i64, i32, i64, i64, i64, vp, i32, f32, f32, f32, i32, i32, i32, vp, ctypes.c_size_t, vp]
    L.fa_kvw8_forward.restype = ctypes.c_int
    pshape = [i64, i32, i32, i64, i64, i32, i32, i32, i32]   # batch, heads_kv, group, nq, nk, d, causal, dtype, window_left
    L.fa_kvw8_paged_workspace_bytes.argtypes = pshape
    L.fa_kvw8_paged_workspace_bytes.restype = ctypes.c_size_t
    L.fa_kvw8_paged_splits_for.argtypes = pshape
    L.fa_kvw8_paged_splits_for.restype = i32
    L.fa_kvw8_paged_forward.argtypes = [vp, ctypes.POINTER(FaPagedCache), vp, vp, i64, i32, i32, i64, i64, i32, f32, f32, f32, i32, i32, i32, vp, ctypes.c_size_t, vp]
    L.fa_kvw8_paged_forward.restype = ctypes.c_int
    L.fa_kvw8_last_error.argtypes = []
    L.fa_kvw8_last_error.restype = ctypes.c_char_p
    L.fa_kvw8_version.argtypes = []
    L.fa_kvw8_version.restype = ctypes.c_char_p
    return L


def lib(path: str = LIB_PATH) -> ctypes.CDLL:
    if path not in _libs:
        if not os.path.exists(path):
            raise ExtensionMissing(
                f"{path} not found. Build it with `python flashattention.c_amd/build.py` "
                "(or __graft_entry__.build()). There is no CPU/PyTorch fallback for this operator.")
        _libs[path] = bind(path)
    return _libs[path]


def check(code: int) -> None:
    if code != FA_OK:
        raise FlashAttnError(code, lib().fa_kvw8_last_error().decode("utf-8", "replace"))
