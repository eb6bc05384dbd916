"""flashattention.c_amd -- MI355X-native fused flash-attention forward behind the reference's ``forward(q, k, v, causal)``.

Layout: ``csrc/`` hand-written HIP kernels + the C ABI (``include/flashattn_amd.h``); ``flash.py`` the host-side mirror
of the reference's Python surface; ``sharding.py`` batch*head sharding; ``build.py`` the hipcc build.
Import name: ``flashattention_c_amd`` (the directory name contains a dot; ``flashattention_c_amd.py`` at the repo root
aliases it).
"""
from . import _cabi, _cabi_ext, _cabi_kv, _cabi_kv8, _cabi_kvw, _cabi_kvw8, _cabi_paged  # noqa: F401
from .flash import KV_HEAD_DIMS, SUPPORTED_HEAD_DIMS, forward, forward_kv, forward_paged, forward_kv_fp8, forward_paged_fp8, forward_packed_qkv, workspace_bytes_kv, workspace_bytes_paged, last_forward_route, load, stats, time_forward, workspace_bytes  # noqa: F401
from .sharding import forward_sharded, shard_range, shard_sizes  # noqa: F401

__all__ = ["forward", "forward_kv", "workspace_bytes_kv", "forward_paged", "workspace_bytes_paged", "forward_kv_fp8", "forward_paged_fp8", "KV_HEAD_DIMS", "forward_packed_qkv", "load", "time_forward", "last_forward_route", "forward_sharded", "shard_range", "shard_sizes", "workspace_bytes",
           "stats", "SUPPORTED_HEAD_DIMS"]
