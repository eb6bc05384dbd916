"""Host-side mirror of the reference's operator surface.

The reference exposes exactly one call (``/root/reference/src/main.cpp:3-6``, used at
``/root/reference/bench_flashattention.py:10,70``)::

    minimal_flash = load(name='flash', sources=[...])
    out = minimal_flash.forward(q, k, v, masking)        # q, k, v: (batch*heads, seq, head_dim) on the GPU

This module provides the same call with the same positional meaning, backed by the C ABI in
``include/flashattn_amd.h`` (hand-written HIP for gfx950).  PyTorch is used for device memory and the stream
handle only.  Defaults reproduce the reference: ``scale = 1.0`` (``flashattention.cu:593,600``), fp32 in -> fp32 out.
Differences, all deliberate (DESIGN.md "boundary"): the call is asynchronous on the current stream (the reference
ends with ``cudaDeviceSynchronize``), invalid input raises ``ValueError``/``TypeError`` instead of tripping a device
``assert`` (``flashattention.cu:606``), every head dim up to 256 runs (32/64/128 on every kernel family, the other multiples of 32
on the exact fp32 kernel -- fp32 or bf16 tensors --, the rest on the rung-0 kernel; the reference needs ``#define d`` edited, ``:15``), any sequence length is exact
(the reference needs N % 32 == 0), and bf16 tensors are accepted (bf16 MFMA path).
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace
from typing import Callable, NamedTuple, Optional, Tuple, Union

import torch

from . import _cabi, _cabi_kv, _cabi_kv8, _cabi_kvw, _cabi_kvw8, _cabi_paged

__all__ = ["forward", "forward_kv", "forward_paged", "forward_kv_fp8", "forward_paged_fp8", "forward_packed_qkv", "load", "time_forward", "last_forward_route", "workspace_bytes", "workspace_bytes_kv",
           "workspace_bytes_paged", "stats",
           "SUPPORTED_HEAD_DIMS", "KV_HEAD_DIMS"]

SUPPORTED_HEAD_DIMS = (32, 64, 128)   # ... by every kernel family; ``kernel="auto"`` takes any head dim up to MAX_HEAD_DIM
MAX_HEAD_DIM = 256
_DTYPES = {torch.float32: _cabi.FA_DTYPE_F32, torch.bfloat16: _cabi.FA_DTYPE_BF16}
_KERNELS = {"auto": _cabi.FA_KERNEL_AUTO, "naive": _cabi.FA_KERNEL_NAIVE, "mfma": _cabi.FA_KERNEL_MFMA,
            "exact": _cabi.FA_KERNEL_MFMA, "split": _cabi.FA_KERNEL_SPLIT, "pb2": _cabi.FA_KERNEL_PB2}


def _kernel_id(kernel: Union[str, int]) -> int:
    if isinstance(kernel, int):
        return kernel
    name, _, variant = kernel.partition(":")
    if name not in _KERNELS:
        raise ValueError(f"unknown kernel {kernel!r}; choose from {sorted(_KERNELS)}")
    return _KERNELS[name] | (int(variant) << 8 if variant else 0)


def _check_qkv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> Tuple[int, int, int]:
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if t.dim() != 3:
            raise ValueError(f"{name} must be 3-D (batch*heads, seq_len, head_dim), got shape {tuple(t.shape)}")
    if not (q.shape == k.shape == v.shape):
        raise ValueError(f"q, k, v must have identical shapes, got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    if not (q.dtype == k.dtype == v.dtype):
        raise TypeError("q, k, v must share one dtype")
    if q.dtype not in _DTYPES:
        raise TypeError(f"dtype {q.dtype} not supported (float32 or bfloat16)")
    if not (q.is_cuda and k.is_cuda and v.is_cuda):
        raise ValueError("q, k, v must live on a GPU (there is no CPU implementation of this operator)")
    if not (q.device == k.device == v.device):
        raise ValueError("q, k, v must be on the same device")
    bh, n, d = q.shape
    if bh < 1 or n < 1:
        raise ValueError("empty batch or sequence")
    return bh, n, d


def _workspace(workspace: Optional[torch.Tensor], need: int, device) -> Optional[torch.Tensor]:
    """the caller's scratch if it will do, else ``need`` bytes from torch's caching allocator (256-byte aligned: its blocks are 512-byte multiples)"""
    if workspace is None:
        return torch.empty(need, dtype=torch.uint8, device=device) if need else None
    if workspace.dtype != torch.uint8 or workspace.device != device or not workspace.is_contiguous() or workspace.numel() < need:
        raise ValueError(f"workspace must be a contiguous torch.uint8 tensor of at least {need} bytes on {device}")
    return workspace


def forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = False, *,
            scale: float = 1.0, return_lse: bool = False, kernel: Union[str, int] = "auto",
            out: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None,
            workspace: Optional[torch.Tensor] = None):
    """``O = softmax(scale * q k^T [+ causal mask]) v`` per (batch*head); drop-in for ``flash.forward(q, k, v, causal)``.

    Returns a new tensor shaped like ``q`` (the reference allocates with ``torch::zeros``; here ``torch.empty`` is
    enough because every element is written).  ``return_lse=True`` additionally returns the (BH, N) fp32 row
    log-sum-exp -- the quantity the reference's unused ``O_l`` buffer was reserved for.

    Kernel choice and accuracy: ``include/flashattn_amd.h`` sections 1-2 are the contract.  fp32 tensors: ``kernel="auto"`` computes on
    the 16-bit matrix pipes with split operands (Q.K^T: two-term fp16 splits of Q' and of the keys centred on a reference key; P.V: two-term
    bf16 splits of P and of the centred values): ``|O - O64| <= max(1e-3, E_ref) + 3 * 2^-17 * max|v - vbar|`` on every input, ``E_ref`` =
    what the reference's own fp32 FMA chain leaves on that input; <= 1e-4 on unit-variance data; a workgroup whose operands leave what the
    16-bit terms hold redoes its rows in fp32 arithmetic inside the same launch.  ``"split"`` is the same without that guard, ``"exact"``
    (= ``"mfma"``) computes in fp32 arithmetic (head dims 32 .. 256 in steps of 32).  bf16 tensors: ``out_dtype=torch.float32`` stores the
    fp32 accumulator and, under ``"auto"``, selects the accurate P -- bf16 hi + bf16 lo terms in one launch (``"pb2"``: 2e-5 on
    B=2 H=8 d=64 N=8192); a bf16 output keeps the fastest kernels (bf16 P, ``"mfma"``: 1.5e-2 there, 3e-4 at 1/sqrt(d)).  Head dims
    outside 32 / 64 / 128: see the module docstring.  ``out`` must not overlap q, k or v.

    The call goes through ``fa_forward_ws``: scratch (the partials of a key-split launch), when the call can use any, is a ``torch.empty``
    byte tensor from torch's caching allocator on the current stream -- the C ABI itself allocates nothing, which also makes every kernel
    family legal under ``torch.cuda.graph`` capture.  ``workspace`` may pass a preallocated ``torch.uint8`` tensor of at least
    ``workspace_bytes(...)`` bytes instead.
    """
    bh, n, d = _check_qkv(q, k, v)
    kid = _kernel_id(kernel)
    if d > MAX_HEAD_DIM:
        raise ValueError(f"head_dim {d} not supported (1 .. {MAX_HEAD_DIM})")
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    if out_dtype is None:
        out_dtype = out.dtype if out is not None else q.dtype
    dt = _DTYPES[q.dtype]
    if out_dtype != q.dtype:
        if not (q.dtype == torch.bfloat16 and out_dtype == torch.float32):
            raise TypeError(f"out_dtype {out_dtype} not supported for {q.dtype} inputs")
        dt = _cabi.FA_DTYPE_BF16_OUT_F32
    if out is None:
        out = torch.empty(q.shape, dtype=out_dtype, device=q.device)
    elif out.shape != q.shape or out.dtype != out_dtype or out.device != q.device or not out.is_contiguous():
        raise ValueError("out must be a contiguous tensor shaped like q with dtype out_dtype")
    lse = torch.empty((bh, n), dtype=torch.float32, device=q.device) if return_lse else None
    L = _cabi.lib()
    with torch.cuda.device(q.device):
        need = int(L.fa_workspace_bytes(bh, n, d, int(bool(causal)), dt, kid))
        workspace = _workspace(workspace, need, q.device)
        stream = torch.cuda.current_stream().cuda_stream
        rc = L.fa_forward_ws(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
                             lse.data_ptr() if lse is not None else None,
                             bh, n, d, float(scale), int(bool(causal)), dt, kid,
                             workspace.data_ptr() if workspace is not None else None,
                             workspace.numel() if workspace is not None else 0, ctypes.c_void_p(stream))
    _cabi.check(rc)
    return (out, lse) if return_lse else out


def workspace_bytes(bh: int, n: int, d: int, causal: bool = False, *, dtype: torch.dtype = torch.float32,
                    out_dtype: Optional[torch.dtype] = None, kernel: Union[str, int] = "auto") -> int:
    """Bytes of scratch ``forward`` needs for this call (``fa_workspace_bytes``); 0 for most shapes."""
    dt = _DTYPES[dtype]
    if out_dtype is not None and out_dtype != dtype:
        dt = _cabi.FA_DTYPE_BF16_OUT_F32
    return int(_cabi.lib().fa_workspace_bytes(int(bh), int(n), int(d), int(bool(causal)), dt, _kernel_id(kernel)))



KV_HEAD_DIMS = (64, 128)

# ---- the four KV-cache entries: one front end.  What differs between a 16-bit and an fp8 cache is the _Family row, what differs between a contiguous
# and a paged cache is the validator (_contiguous_cache / _paged_cache); library and symbols follow from (fp8?, paged?, window?) in _ENTRIES ----


def _check_bf16_cache(fn: str, q, kn: str, k, vn: str, v, table=None) -> None:
    """dtype and device checks of the two 16-bit entries: bf16 q and caches on one GPU, the block table with them."""
    if not (q.dtype == k.dtype == v.dtype):
        raise TypeError(f"q, {kn}, {vn} must share one dtype")
    if q.dtype != torch.bfloat16:
        raise TypeError(f"dtype {q.dtype} not supported by {fn} (bfloat16: caches are 16-bit)")
    if table is None:
        if not (q.is_cuda and k.is_cuda and v.is_cuda) or not (q.device == k.device == v.device):
            raise ValueError("q, k, v must live on the same GPU (there is no CPU implementation of this operator)")
    elif not (q.is_cuda and k.is_cuda and v.is_cuda and table.is_cuda) or not (q.device == k.device == v.device == table.device):
        raise ValueError("q, the pools and the block table must live on the same GPU (there is no CPU implementation of this operator)")


def _check_fp8_cache(fn: str, q, kn: str, k, vn: str, v, table=None) -> None:
    """dtype and device checks of the two fp8 entries: bf16 q, e4m3fn caches on q's GPU, the block table with them."""
    for name, t in ((kn, k), (vn, v)):
        if t.dtype == torch.uint8:
            raise TypeError(f"{name} is torch.uint8: {fn} takes torch.float8_e4m3fn -- reinterpret the bytes with {name}.view(torch.float8_e4m3fn)")
        if t.dtype != torch.float8_e4m3fn:
            raise TypeError(f"dtype {t.dtype} of {name} not supported by {fn} (torch.float8_e4m3fn)")
    if q.dtype != torch.bfloat16:
        raise TypeError(f"dtype {q.dtype} of q not supported by {fn} (bfloat16)")
    if not (q.is_cuda and k.is_cuda and v.is_cuda) or not (q.device == k.device == v.device):
        raise ValueError("q and the cache must live on the same GPU (there is no CPU implementation of this operator)")
    if table is not None and (not table.is_cuda or table.device != q.device):
        raise ValueError("q, the pools and the block table must live on the same GPU (there is no CPU implementation of this operator)")


class _Family(NamedTuple):
    """what an element type of the cache changes in the front end"""
    fp8: bool
    contiguous: Tuple[str, str, str]   # the contiguous entry and its cache arguments, as messages name them
    paged: Tuple[str, str, str]        # the paged entry and its pools
    stride_multiple: int               # pool strides come in multiples of 16 bytes: this many elements
    check_dtypes_and_devices: Callable


_OUT_BF16 = {torch.bfloat16: _cabi.FA_DTYPE_BF16}   # out_dtype -> the C ABI's dtype code; everything else stores the fp32 accumulator
_BF16 = _Family(False, ("forward_kv", "k", "v"), ("forward_paged", "k_pool", "v_pool"), 8, _check_bf16_cache)
_FP8 = _Family(True, ("forward_kv_fp8", "k8", "v8"), ("forward_paged_fp8", "k_pool8", "v_pool8"), 16, _check_fp8_cache)

# (fp8?, paged?, window?) -> the binding, its forward, its workspace query
_ENTRIES = {
    (False, False, False): (_cabi_kv, "fa_kv_forward", "fa_kv_workspace_bytes"),
    (False, True, False): (_cabi_paged, "fa_paged_forward", "fa_paged_workspace_bytes"),
    (True, False, False): (_cabi_kv8, "fa_kv8_forward", "fa_kv8_workspace_bytes"),
    (True, True, False): (_cabi_kv8, "fa_kv8_paged_forward", "fa_kv8_workspace_bytes"),   # no paged query there: the contiguous one at batch * heads_kv
    (False, False, True): (_cabi_kvw, "fa_kvw_forward", "fa_kvw_workspace_bytes"),
    (False, True, True): (_cabi_kvw, "fa_kvw_paged_forward", "fa_kvw_paged_workspace_bytes"),
    (True, False, True): (_cabi_kvw8, "fa_kvw8_forward", "fa_kvw8_workspace_bytes"),
    (True, True, True): (_cabi_kvw8, "fa_kvw8_paged_forward", "fa_kvw8_paged_workspace_bytes"),
}


def _window(window_left: Optional[int]) -> Optional[int]:
    """``window_left`` as the windowed entries take it: None (no window: the unwindowed libraries), or an int in 0 .. 2^24 (wider hides nothing)"""
    if window_left is None:
        return None
    if isinstance(window_left, bool) or not isinstance(window_left, int):
        raise TypeError(f"window_left must be None or an int, got {type(window_left).__name__}")
    if window_left < 0:
        raise ValueError(f"window_left = {window_left} must be >= 0 (None: no window)")
    return min(window_left, 1 << 24)


def _lens(name: str, lens: torch.Tensor, n: int, device) -> int:
    """device pointer of ``kv_lens`` / ``seq_lens``: int32 ``(n,)`` on ``device``"""
    if not isinstance(lens, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if lens.dtype != torch.int32 or lens.shape != (n,) or lens.device != device or not lens.is_contiguous():
        raise ValueError(f"{name} must be a contiguous torch.int32 tensor of shape ({n},) on {device}")
    return lens.data_ptr()


def _contiguous_cache(fam: _Family, q, k, v, kv_len, kv_lens):
    """Validate q against a contiguous cache.  Returns q, k, v made contiguous, the shape as the queries take it (bh_kv, group, nq, nk, d)
    and what a forward takes between ``lse`` and ``scale``."""
    fn, kn, vn = fam.contiguous
    for name, t in (("q", q), (kn, k), (vn, v)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if t.dim() != 3:
            raise ValueError(f"{name} must be 3-D (batch*heads, rows, head_dim), got shape {tuple(t.shape)}")
    if k.shape != v.shape:
        raise ValueError(f"{kn} and {vn} must have identical shapes, got {tuple(k.shape)}, {tuple(v.shape)}")
    fam.check_dtypes_and_devices(fn, q, kn, k, vn, v)
    bhq, nq, d = q.shape
    bhkv, capacity, dk = k.shape
    if dk != d:
        raise ValueError(f"head_dim of q ({d}) and of {kn}, {vn} ({dk}) differ")
    if d not in KV_HEAD_DIMS:
        raise ValueError(f"head_dim {d} not supported by {fn} (choose from {KV_HEAD_DIMS})")
    if bhq < 1 or nq < 1 or bhkv < 1 or capacity < 1:
        raise ValueError("empty batch or sequence")
    if bhq % bhkv != 0:
        raise ValueError(f"q has {bhq} slabs, {kn} / {vn} have {bhkv}: not a whole number of query heads per K/V head")
    group = bhq // bhkv
    nk = capacity if kv_len is None else int(kv_len)
    if not 1 <= nk <= capacity:
        raise ValueError(f"kv_len {nk} outside 1 .. capacity = {capacity}")
    lens = None if kv_lens is None else _lens("kv_lens", kv_lens, bhkv, q.device)
    return q.contiguous(), k.contiguous(), v.contiguous(), (bhkv, group, nq, nk, d), (bhkv, group, nq, nk, capacity, lens, d)


def _paged_cache(fam: _Family, q, k_pool, v_pool, block_table, kv_len, seq_lens):
    """Validate q against pools under a block table (a pool is never copied).  Returns q made contiguous, the ``fa_paged_cache`` and the
    shape (batch, heads_kv, group, nq, nk, d): what the queries take, and a forward between ``lse`` and ``scale``."""
    fn, kn, vn = fam.paged
    for name, t in (("q", q), (kn, k_pool), (vn, v_pool), ("block_table", block_table)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    if q.dim() != 3:
        raise ValueError(f"q must be 3-D (batch*heads, rows, head_dim), got shape {tuple(q.shape)}")
    if k_pool.dim() not in (3, 4):
        raise ValueError(f"{kn} must be (pages, page, d) or (pages, page, H, d), got shape {tuple(k_pool.shape)}")
    if k_pool.shape != v_pool.shape or k_pool.stride() != v_pool.stride():
        raise ValueError(f"{kn} and {vn} must have identical shapes and strides, got {tuple(k_pool.shape)} / {k_pool.stride()} and "
                         f"{tuple(v_pool.shape)} / {v_pool.stride()}")
    fam.check_dtypes_and_devices(fn, q, kn, k_pool, vn, v_pool, block_table)
    bhq, nq, d = q.shape
    pages, page = k_pool.shape[0], k_pool.shape[1]
    heads_kv = k_pool.shape[2] if k_pool.dim() == 4 else 1
    if k_pool.shape[-1] != d:
        raise ValueError(f"head_dim of q ({d}) and of the pools ({k_pool.shape[-1]}) differ")
    if d not in KV_HEAD_DIMS:
        raise ValueError(f"head_dim {d} not supported by {fn} (choose from {KV_HEAD_DIMS})")
    if k_pool.stride(-1) != 1:
        raise ValueError(f"the pools' last stride must be 1, got {k_pool.stride(-1)} (a pool is never copied)")
    page_stride, row_stride = k_pool.stride(0), k_pool.stride(1)
    head_stride = k_pool.stride(2) if k_pool.dim() == 4 else 0
    m = fam.stride_multiple
    if page_stride % m or row_stride % m or head_stride % m:
        raise ValueError(f"pool strides must be multiples of {m} elements (16 bytes), got {k_pool.stride()} (a pool is never copied)")
    if block_table.dim() != 2 or block_table.dtype != torch.int32 or not block_table.is_contiguous():
        raise ValueError("block_table must be a contiguous torch.int32 tensor of shape (batch, max_pages)")
    batch, max_pages = block_table.shape
    if bhq < 1 or nq < 1 or batch < 1 or max_pages < 1 or pages < 1 or heads_kv < 1:
        raise ValueError("empty batch, sequence, pool or block table")
    if bhq % (batch * heads_kv) != 0:
        raise ValueError(f"q has {bhq} slabs, the cache {batch} sequences x {heads_kv} heads: not a whole number of query heads per K/V head")
    group = bhq // (batch * heads_kv)
    nk = max_pages * page if kv_len is None else int(kv_len)
    if not 1 <= nk <= max_pages * page:
        raise ValueError(f"kv_len {nk} outside 1 .. max_pages * page = {max_pages * page}")
    cache = _cabi_paged.FaPagedCache(k_pool.data_ptr(), v_pool.data_ptr(), pages, page, page_stride, row_stride, head_stride,
                                     block_table.data_ptr(), max_pages, None if seq_lens is None else _lens("seq_lens", seq_lens, batch, q.device))
    return q.contiguous(), cache, (batch, heads_kv, group, nq, nk, d)


def _workspace_need(fp8: bool, paged: bool, shape, causal: int, dt: int, window: tuple) -> int:
    """``*_workspace_bytes`` of the library that runs (fp8?, paged?, window?) for ``shape`` as that query takes it; ``window``: () or (window_left,)"""
    mod, _, query = _ENTRIES[fp8, paged, bool(window)]
    if fp8 and paged and not window:
        shape = (shape[0] * shape[1], *shape[2:])
    return int(getattr(mod.lib(), query)(*shape, causal, dt, *window))


def _out_lse_workspace(q, out, out_dtype, return_lse, workspace, need):
    """out, lse and workspace as the four entries prepare them"""
    if out_dtype is None:
        out_dtype = out.dtype if out is not None else q.dtype
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"out_dtype {out_dtype} not supported for {q.dtype} inputs")
    if out is None:
        out = torch.empty(q.shape, dtype=out_dtype, device=q.device)
    elif out.shape != q.shape or out.dtype != out_dtype or out.device != q.device or not out.is_contiguous():
        raise ValueError("out must be a contiguous tensor shaped like q with dtype out_dtype")
    lse = torch.empty(q.shape[:2], dtype=torch.float32, device=q.device) if return_lse else None
    return out, lse, _workspace(workspace, need, q.device)


def _run(fam: _Family, paged: bool, window_left, q, cache, shape, dims, scale, scales, causal, return_lse, out, out_dtype, workspace):
    """The call of (family, paged?, window?): ``cache`` is what a forward takes between ``q`` and ``o`` (two pointers, or the fa_paged_cache),
    ``shape`` what the workspace query takes, ``dims`` what the forward takes between ``lse`` and ``scale``, ``scales`` the fp8 pair or ()."""
    window = () if window_left is None else (window_left,)
    causal = int(bool(causal))
    mod, forward, _ = _ENTRIES[fam.fp8, paged, window_left is not None]
    index = q.device.index   # device and stream by index: torch resolves a torch.device, or no device at all, through a slow path on every call
    with torch.cuda.device(index):
        dt = _OUT_BF16.get(out_dtype if out_dtype is not None else (out.dtype if out is not None else q.dtype), _cabi.FA_DTYPE_BF16_OUT_F32)
        need = _workspace_need(fam.fp8, paged, shape, causal, dt, window)
        out, lse, workspace = _out_lse_workspace(q, out, out_dtype, return_lse, workspace, need)
        if scales:
            scales = (float(scales[0]), float(scales[1]))
        stream = torch.cuda.current_stream(index).cuda_stream
        rc = getattr(mod.lib(), forward)(q.data_ptr(), *cache, out.data_ptr(), lse.data_ptr() if lse is not None else None, *dims,
                                         float(scale), *scales, causal, dt, *window,
                                         workspace.data_ptr() if workspace is not None and workspace.numel() else None,
                                         workspace.numel() if workspace is not None else 0, ctypes.c_void_p(stream))
    mod.check(rc)
    return (out, lse) if return_lse else out


def forward_kv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = False, *, kv_len: Optional[int] = None,
               kv_lens: Optional[torch.Tensor] = None, scale: float = 1.0, return_lse: bool = False, out: Optional[torch.Tensor] = None,
               out_dtype: Optional[torch.dtype] = None, workspace: Optional[torch.Tensor] = None, window_left: Optional[int] = None):
    """Attention of few query rows against a K/V cache (``include/flashattn_amd_kv.h``): decode, chunked prefill, cross-attention, GQA.

    ``q`` is ``(BHq, nq, d)``; ``k``, ``v`` are ``(BHkv, capacity, d)`` caches of which the first ``kv_len`` rows (default: all ``capacity``)
    are attended to; ``BHq = BHkv * group``, query slab ``s`` reads K/V slab ``s // group``.  ``kv_lens``, an int32 tensor ``(BHkv,)`` on the
    device, gives each slab its own length (clamped to ``[0, kv_len]``); it is read by the kernel, never by the host, so a captured graph can
    be replayed while the cache grows.  ``causal`` is bottom-right aligned: query row ``i`` sees keys ``j <= len - nq + i``.  Rows without a
    visible key get ``O = 0``, ``LSE = -inf``.  bfloat16 tensors, ``d`` 64 or 128; ``out_dtype=torch.float32`` stores the fp32 accumulator.
    Arithmetic and accuracy are those of ``forward(..., out_dtype=torch.float32)`` on bf16 tensors (P as two bf16 terms) for both outputs.
    Scratch (``workspace_bytes_kv``; key-split launches only) comes from ``torch.empty`` unless ``workspace`` passes a ``torch.uint8`` tensor.

    ``window_left`` (``include/flashattn_amd_kvw.h``; ``None``: no window) is a sliding window, read as flash-attn's ``window_size=(left, -1 | 0)``:
    with ``len`` a slab's length, query row ``i`` sees key ``j`` iff ``j < len``, ``j >= len - nq + i - window_left`` and, when ``causal``,
    ``j <= len - nq + i`` -- causal with ``window_left = W - 1`` is "the last ``W`` keys including my own".  An ``int >= 0``; negative raises
    ``ValueError``.  The call walks only the keys of the window, so its time follows ``window_left``, not ``len``, and with
    ``lo = max(0, len - nq - window_left)`` no K/V row below ``lo`` and none at or beyond ``len`` is ever read: rows that have slid out of
    the window may hold anything.  Pass the same ``window_left`` to ``workspace_bytes_kv``.
    """
    window_left = _window(window_left)
    q, k, v, shape, dims = _contiguous_cache(_BF16, q, k, v, kv_len, kv_lens)
    return _run(_BF16, False, window_left, q, (k.data_ptr(), v.data_ptr()), shape, dims, scale, (), causal, return_lse, out, out_dtype, workspace)


def workspace_bytes_kv(bh_kv: int, group: int, nq: int, nk: int, d: int, causal: bool = False, *, out_dtype: torch.dtype = torch.bfloat16,
                       window_left: Optional[int] = None) -> int:
    """Bytes of scratch ``forward_kv`` can use for these shapes (``fa_kv_workspace_bytes``) and this ``window_left`` (``fa_kvw_workspace_bytes``:
    the plan is laid over ``min(nk, window_left + nq + 63)`` keys); 0 when the plan does not split the keys."""
    window_left = _window(window_left)
    return _workspace_need(False, False, (int(bh_kv), int(group), int(nq), int(nk), int(d)), int(bool(causal)),
                           _OUT_BF16.get(out_dtype, _cabi.FA_DTYPE_BF16_OUT_F32), () if window_left is None else (window_left,))


def forward_paged(q: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor, causal: bool = False, *,
                  seq_lens: Optional[torch.Tensor] = None, kv_len: Optional[int] = None, scale: float = 1.0, return_lse: bool = False,
                  out: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None, workspace: Optional[torch.Tensor] = None,
                  window_left: Optional[int] = None):
    """``forward_kv`` over a paged cache (``include/flashattn_amd_paged.h``): K/V rows live in pages of a shared pool, found through a block table.

    ``k_pool``, ``v_pool`` are ``(pages, page, d)`` (one K/V head) or ``(pages, page, H, d)``; their strides are taken as they are, so a
    ``(pages, H, page, d).permute(0, 2, 1, 3)`` view works without a copy -- a pool is never copied: a last stride other than 1 or a stride that
    is not a multiple of 8 elements raises.  ``block_table`` is int32 ``(batch, max_pages)`` on the device: entry ``p`` of sequence ``b`` is the
    physical page of its rows ``[p * page, (p + 1) * page)``.  ``q`` is ``(batch * H * group, nq, d)``; query slab ``((b * H) + h) * group + g``
    reads head ``h`` of sequence ``b``.  ``kv_len`` (default ``max_pages * page``) bounds every sequence; ``seq_lens``, int32 ``(batch,)`` on the
    device, gives each its own length (clamped to ``[0, kv_len]``).  Table and lengths are read by the kernel only, so one captured graph
    follows a cache that grows and whose pages move.  Pages of 16 .. 65536 rows, a power of two.  Everything else -- ``causal``, rows without
    keys, dtypes, arithmetic, scratch (``workspace_bytes_paged``) -- is ``forward_kv``'s, and so is the result, bit for bit, on the gathered cache.

    ``window_left`` (``None``: no window) is ``forward_kv``'s sliding window: row ``i`` sees key ``j`` iff ``j < len``, ``j >= len - nq + i - window_left``
    and, when ``causal``, ``j <= len - nq + i``.  With ``lo = max(0, len - nq - window_left)`` no pool row of a key below ``lo`` or at or beyond
    ``len`` is read, and no table entry below ``lo // page`` or at or beyond ``ceil(len / page)``: pages that have slid out of the window can be
    freed or reused, and their entries may hold anything.  Pass the same ``window_left`` to ``workspace_bytes_paged``.
    """
    window_left = _window(window_left)
    q, cache, shape = _paged_cache(_BF16, q, k_pool, v_pool, block_table, kv_len, seq_lens)
    return _run(_BF16, True, window_left, q, (ctypes.byref(cache),), shape, shape, scale, (), causal, return_lse, out, out_dtype, workspace)


def workspace_bytes_paged(batch: int, heads_kv: int, group: int, nq: int, nk: int, d: int, causal: bool = False, *,
                          out_dtype: torch.dtype = torch.bfloat16, window_left: Optional[int] = None) -> int:
    """Bytes of scratch ``forward_paged`` can use for these shapes (``fa_paged_workspace_bytes`` = ``workspace_bytes_kv`` at ``batch * heads_kv``)
    and this ``window_left`` (``fa_kvw_paged_workspace_bytes``)."""
    window_left = _window(window_left)
    return _workspace_need(False, True, (int(batch), int(heads_kv), int(group), int(nq), int(nk), int(d)), int(bool(causal)),
                           _OUT_BF16.get(out_dtype, _cabi.FA_DTYPE_BF16_OUT_F32), () if window_left is None else (window_left,))


def forward_kv_fp8(q: torch.Tensor, k8: torch.Tensor, v8: torch.Tensor, causal: bool = False, *, k_scale: float = 1.0, v_scale: float = 1.0,
                   kv_len: Optional[int] = None, kv_lens: Optional[torch.Tensor] = None, scale: float = 1.0, return_lse: bool = False,
                   out: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None, workspace: Optional[torch.Tensor] = None,
                   window_left: Optional[int] = None):
    """``forward_kv`` over a cache of 8-bit floats (``include/flashattn_amd_kv8.h``): half the K/V bytes of a call.

    ``q`` is bfloat16 ``(BHq, nq, d)``; ``k8``, ``v8`` are ``torch.float8_e4m3fn`` ``(BHkv, capacity, d)`` (a ``torch.uint8`` tensor is rejected:
    ``.view(torch.float8_e4m3fn)`` it).  Logical K = ``k_scale`` x the stored values, logical V = ``v_scale`` x them: one positive float per
    tensor and call.  The kernel dequantises to bf16 exactly and runs the arithmetic of ``forward_kv``; ``k_scale`` is folded into ``scale`` as
    one fp32 product, ``v_scale`` multiplies the normalised result once, the LSE is that of the scaled scores.  With ``v_scale`` a power of two
    the result is bit for bit ``v_scale * forward_kv(q, k8.to(bfloat16), v8.to(bfloat16), scale=fp32(scale * k_scale))``.  Everything else --
    ``kv_len``, ``kv_lens``, ``causal``, rows without keys, ``d``, output dtypes -- is ``forward_kv``'s; scratch has the size ``workspace_bytes_kv``
    gives for the same shapes and ``window_left``.

    ``window_left`` (``include/flashattn_amd_kvw8.h``; ``None``: no window) is ``forward_kv``'s sliding window with its rules: an ``int >= 0``
    (negative raises ``ValueError``), only the keys of the window are walked, and with ``lo = max(0, len - nq - window_left)`` no cache byte of a
    row below ``lo`` or at or beyond ``len`` is read -- such rows may hold anything, the NaN codes included.  With ``v_scale`` a power of two the
    result is bit for bit ``v_scale *`` that of ``forward_kv`` on the dequantised cache with the same ``window_left``.
    """
    window_left = _window(window_left)
    q, k8, v8, shape, dims = _contiguous_cache(_FP8, q, k8, v8, kv_len, kv_lens)
    return _run(_FP8, False, window_left, q, (k8.data_ptr(), v8.data_ptr()), shape, dims, scale, (k_scale, v_scale), causal, return_lse, out, out_dtype,
                workspace)


def forward_paged_fp8(q: torch.Tensor, k_pool8: torch.Tensor, v_pool8: torch.Tensor, block_table: torch.Tensor, causal: bool = False, *,
                      k_scale: float = 1.0, v_scale: float = 1.0, seq_lens: Optional[torch.Tensor] = None, kv_len: Optional[int] = None,
                      scale: float = 1.0, return_lse: bool = False, out: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None,
                      workspace: Optional[torch.Tensor] = None, window_left: Optional[int] = None):
    """``forward_paged`` over pools of 8-bit floats (``include/flashattn_amd_kv8.h``); scales and arithmetic as in ``forward_kv_fp8``.

    ``k_pool8``, ``v_pool8`` are ``torch.float8_e4m3fn`` ``(pages, page, d)`` or ``(pages, page, H, d)`` (``torch.uint8`` is rejected: ``.view`` it).
    Their strides are taken as they are and a pool is never copied: a last stride other than 1 or a stride that is not a multiple of 16
    elements (16 bytes) raises.  Block table, ``seq_lens``, ``kv_len``, page sizes and everything else are ``forward_paged``'s, and the result is
    ``forward_kv_fp8``'s, bit for bit, on the gathered bytes; scratch has the size ``workspace_bytes_paged`` gives for the same shapes and
    ``window_left``.

    ``window_left`` (``include/flashattn_amd_kvw8.h``; ``None``: no window) is ``forward_paged``'s sliding window: with
    ``lo = max(0, len - nq - window_left)`` no pool byte of a key below ``lo`` or at or beyond ``len`` is read, and no table entry below
    ``lo // page`` or at or beyond ``ceil(len / page)``: pages that have slid out can be freed or reused and may hold NaN codes.
    """
    window_left = _window(window_left)
    q, cache, shape = _paged_cache(_FP8, q, k_pool8, v_pool8, block_table, kv_len, seq_lens)
    return _run(_FP8, True, window_left, q, (ctypes.byref(cache),), shape, shape, scale, (k_scale, v_scale), causal, return_lse, out, out_dtype, workspace)


def forward_packed_qkv(inp: torch.Tensor, n_head: int) -> torch.Tensor:
    """llm.c layout: ``inp`` (B, T, 3C) fp32 -> (B, T, C); causal, scale 1/sqrt(C/n_head).

    Replaces ``attention_forward6`` (/root/reference/src/llm.c/attention_forward.cu:1106-1179) without its
    permute / unpermute kernels or temporaries.
    """
    if inp.dim() != 3 or inp.shape[-1] % 3 != 0:
        raise ValueError(f"inp must be (B, T, 3C), got {tuple(inp.shape)}")
    if inp.dtype != torch.float32 or not inp.is_cuda:
        raise TypeError("inp must be a float32 GPU tensor")
    b, t, c3 = inp.shape
    c = c3 // 3
    if c % n_head != 0:
        raise ValueError("C must be divisible by n_head")
    inp = inp.contiguous()
    out = torch.empty((b, t, c), dtype=torch.float32, device=inp.device)
    with torch.cuda.device(inp.device):
        stream = torch.cuda.current_stream().cuda_stream
        rc = _cabi.lib().fa_forward_packed_qkv(inp.data_ptr(), out.data_ptr(), b, t, c, int(n_head), ctypes.c_void_p(stream))
    _cabi.check(rc)
    return out


def time_forward(q, k, v, causal: bool = False, *, scale: float = 1.0, kernel: Union[str, int] = "auto",
                 warmup: int = 3, iters: int = 20, out: Optional[torch.Tensor] = None, graph: bool = False) -> float:
    """Mean milliseconds per forward, HIP events recorded on the launch stream inside the C ABI (fa_time_forward).
    ``graph=True``: the ``iters`` launches are captured into one hipGraph and one replay is timed (fa_time_forward_graph)."""
    bh, n, d = _check_qkv(q, k, v)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    if out is None:
        out = torch.empty_like(q)
    dt = _DTYPES[q.dtype]
    if out.dtype != q.dtype:
        if not (q.dtype == torch.bfloat16 and out.dtype == torch.float32):
            raise TypeError(f"out dtype {out.dtype} not supported for {q.dtype} inputs")
        dt = _cabi.FA_DTYPE_BF16_OUT_F32
    ms = ctypes.c_float(0.0)
    with torch.cuda.device(q.device):
        if graph:
            torch.cuda.current_stream().synchronize()
            rc = _cabi.lib().fa_time_forward_graph(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), bh, n, d, float(scale),
                                                   int(bool(causal)), dt, _kernel_id(kernel), int(warmup), int(iters),
                                                   ctypes.byref(ms))
            _cabi.check(rc)
            return float(ms.value)
        stream = torch.cuda.current_stream().cuda_stream
        rc = _cabi.lib().fa_time_forward(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), bh, n, d, float(scale),
                                         int(bool(causal)), dt, _kernel_id(kernel), ctypes.c_void_p(stream),
                                         int(warmup), int(iters), ctypes.byref(ms))
    _cabi.check(rc)
    return float(ms.value)


def last_forward_route(stream: Optional[torch.cuda.Stream] = None) -> int:
    """Which arithmetic produced this thread's most recent forward (blocking; diagnostics): 0 = nothing to report (every bf16 path,
    explicit kernels, other head dims, forwards enqueued under graph capture), 1 = fp32 tensors under ``"auto"``: split products throughout,
    2 = the range guard fired (operands outside what fp16 terms hold, or a NaN) and at least one workgroup redid its rows in exact fp32
    arithmetic (inside the same launch)."""
    r = ctypes.c_int32(0)
    s = (stream or torch.cuda.current_stream()).cuda_stream
    _cabi.check(_cabi.lib().fa_last_forward_route(ctypes.c_void_p(s), ctypes.byref(r)))
    return int(r.value)


def stats() -> dict:
    """Host counters (``fa_get_stats``: forwards, re-plans without scratch) merged with the two counters the kernels bump on their slow
    paths (``fa_read_device_counters``, BLOCKING): ``tiles_redone`` (optimistic attempt failed, tile recomputed: ~2x) and
    ``workgroups_fp32`` (fp32 ``"auto"`` workgroups redone in fp32 arithmetic: ~3x)."""
    st = _cabi.FaStats()
    _cabi.check(_cabi.lib().fa_get_stats(ctypes.byref(st), ctypes.sizeof(st)))
    out = {n: int(getattr(st, n)) for n, _ in _cabi.FaStats._fields_}
    t, w = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _cabi.check(_cabi.lib().fa_read_device_counters(ctypes.byref(t), ctypes.byref(w)))
    out["tiles_redone"], out["workgroups_fp32"] = int(t.value), int(w.value)
    return out


def load(name: str = "flash", sources=None, extra_cuda_cflags=None, **_ignored):
    """Stand-in for ``torch.utils.cpp_extension.load(name='flash', sources=[...])`` as called at
    /root/reference/bench_flashattention.py:10: returns an object whose ``.forward(q, k, v, causal)`` is this operator.
    ``sources`` / flags are accepted and ignored -- the library is prebuilt by ``build.py``."""
    _cabi.lib()  # fail loudly now if the extension is missing
    return SimpleNamespace(forward=forward, forward_packed_qkv=forward_packed_qkv, __name__=name)
