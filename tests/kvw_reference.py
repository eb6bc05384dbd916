"""fp64 reference of the sliding-window KV-cache forward (include/flashattn_amd_kvw.h): tests/kv_reference.attention_kv plus the lower bound;
tests/test_kvw_host.py pins it to attention_kv."""
import numpy as np


def lo_slab(length, nq, window_left):
    """the first K/V row a slab of this length may be read at"""
    return max(0, int(length) - nq - window_left)


def attention_kvw(q, k, v, lens=None, causal=False, scale=1.0, window_left=0):
    """q (BHq, nq, d); k, v (BHkv, nk, d); lens: per K/V slab, None = nk.  Query i sees key j iff j < len, j >= len - nq + i - window_left and,
    causal, j <= len - nq + i.  Returns O (BHq, nq, d) and LSE (BHq, nq), fp64.  Rows of k, v no query may see are never used (NaN there is
    harmless, as on the device)."""
    q, k, v = (np.asarray(t, dtype=np.float64) for t in (q, k, v))
    group, nq, nk = q.shape[0] // k.shape[0], q.shape[1], k.shape[1]
    lens = np.full(k.shape[0], nk) if lens is None else np.clip(np.asarray(lens), 0, nk)
    ln = np.repeat(lens, group)[:, None, None]                                   # K/V slab s // group serves query slab s
    j, i = np.arange(nk)[None, None, :], np.arange(nq)[None, :, None]
    seen = (j < ln) & (j >= ln - nq + i - window_left) & ((j <= ln - nq + i) if causal else True)
    used = np.repeat(seen.any(axis=1)[:, :, None], k.shape[2], axis=2)          # (BHq, nk, d): keys some row of the slab sees
    kk, vv = np.where(used, np.repeat(k, group, axis=0), 0.0), np.where(used, np.repeat(v, group, axis=0), 0.0)
    s = np.where(seen, scale * np.einsum("bid,bjd->bij", q, kk), -np.inf)
    m = s.max(axis=-1, keepdims=True)
    p = np.exp(s - np.where(np.isfinite(m), m, 0.0))                              # a row without keys: all zeros
    l = p.sum(axis=-1, keepdims=True)
    o = np.einsum("bij,bjd->bid", p, vv) / np.where(l > 0, l, 1.0)
    with np.errstate(divide="ignore"):
        return o, (np.where(np.isfinite(m), m, 0.0) + np.log(l))[..., 0]
