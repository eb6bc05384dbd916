"""ctypes views of the KV-cache extension libraries (include/flashattn_amd_kv.h, _paged.h, _kv8.h, _kvw.h, _kvw8.h), described once.

The five headers are made of the same blocks: a shape tuple (contiguous or paged) that the queries take, a forward whose head and tail are
fixed and whose middle grows by ``k_scale, v_scale`` (fp8 caches) and by ``window_left`` (sliding window), and a ``*_kernel_name_for`` that
takes ``page_size`` where the library has paged kernels.  ``_cabi_kv.py`` .. ``_cabi_kvw8.py`` put their library together from these blocks
and keep the names everything else imports; the loader (``bind``, ``lib``, ``check``) lives here.
"""
from __future__ import annotations

import ctypes
import os

from ._cabi import FA_OK, ExtensionMissing, FlashAttnError

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
vp, i32, i64, f32, size_t, c_int, c_str = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p


class FaPagedCache(ctypes.Structure):
    """``fa_paged_cache`` (include/flashattn_amd_paged.h): the pools, their strides (elements), the block table and the lengths (device
    pointers).  The fp8 libraries read the same struct, its pools as e4m3 bytes."""
    _fields_ = [("k_pool", ctypes.c_void_p), ("v_pool", ctypes.c_void_p), ("num_pages", ctypes.c_int64), ("page_size", ctypes.c_int32),
                ("page_stride", ctypes.c_int64), ("row_stride", ctypes.c_int64), ("head_stride", ctypes.c_int64),
                ("block_table", ctypes.c_void_p), ("max_pages", ctypes.c_int32), ("seq_lens", ctypes.c_void_p)]


SHAPE = [i64, i32, i64, i64, i32, i32, i32]              # bh_kv, group, nq, nk, d, causal, dtype
PAGED_SHAPE = [i64, i32, i32, i64, i64, i32, i32, i32]   # batch, heads_kv, group, nq, nk, d, causal, dtype
WINDOW = [i32]                                           # + window_left: after the shape of a query, after dtype in a forward
PAGE_SIZE = [i32]                                        # + page_size: after the shape of a *_kernel_name_for


def forward_args(paged: bool = False, fp8: bool = False, window: bool = False) -> list:
    """q, the cache, o, lse, the dimensions, scale [, k_scale, v_scale], causal, dtype [, window_left], workspace, workspace_bytes, stream"""
    head = [vp, ctypes.POINTER(FaPagedCache), vp, vp, i64, i32, i32, i64, i64, i32] if paged else [vp, vp, vp, vp, vp, i64, i32, i64, i64, i64, vp, i32]
    return head + [f32] + ([f32, f32] if fp8 else []) + [i32, i32] + (WINDOW if window else []) + [vp, size_t, vp]


def queries(shape: list, name_shape: list, paged: str = "") -> list:
    """the three shape queries of a library (``paged="paged_"``: its paged pair, which has no kernel_name_for of its own)"""
    return [(paged + "workspace_bytes", shape, size_t), (paged + "splits_for", shape, i32)] + ([] if paged else [("kernel_name_for", name_shape, c_str)])


class Extension:
    """One library: ``prototypes`` is [(name without the prefix, argtypes, restype)] in the order of its header; every library ends with
    ``<prefix>last_error`` and ``<prefix>version``."""

    def __init__(self, tag: str, prototypes: list):
        self.prefix = f"fa_{tag}_"
        self.LIB_PATH = os.path.join(PKG_DIR, f"libflashattn_amd_{tag}.so")
        self.prototypes = [(self.prefix + n, a, r) for n, a, r in prototypes + [("last_error", [], c_str), ("version", [], c_str)]]
        self.EXPORTED_SYMBOLS = tuple(n for n, _, _ in self.prototypes)
        self._libs = {}

    def bind(self, path: str) -> ctypes.CDLL:
        """Load a build of the library and declare its prototypes (profiles/kv_decode.py binds measurement builds beside the product)."""
        L = ctypes.CDLL(path)
        for name, argtypes, restype in self.prototypes:
            f = getattr(L, name)
            f.argtypes, f.restype = argtypes, restype
        return L

    def lib(self, path: str = None) -> ctypes.CDLL:
        path = path or self.LIB_PATH
        if path not in self._libs:
            if not os.path.exists(path):
                raise ExtensionMissing(
                    f"{path} not found. Build it with `python flashattention.c_amd/build.py` "
                    "(or __graft_entry__.build()). There is no CPU/PyTorch fallback for this operator.")
            self._libs[path] = self.bind(path)
        return self._libs[path]

    def check(self, code: int) -> None:
        """raise with the text of THIS library's thread-local error"""
        if code != FA_OK:
            raise FlashAttnError(code, getattr(self.lib(), self.prefix + "last_error")().decode("utf-8", "replace"))
