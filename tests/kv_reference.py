"""fp64 reference of the KV-cache forward (include/flashattn_amd_kv.h); tests/test_kv_host.py pins it to oracle.attention_f64."""
import numpy as np


def attention_kv(q, k, v, lens=None, causal=False, scale=1.0):
    """q (BHq, nq, d); k, v (BHkv, nk, d); lens: per K/V slab, None = nk.  Returns O (BHq, nq, d) and LSE (BHq, nq), fp64."""
    q, k, v = (np.asarray(t, dtype=np.float64) for t in (q, k, v))
    group, nq, nk = q.shape[0] // k.shape[0], q.shape[1], k.shape[1]
    lens = np.full(k.shape[0], nk) if lens is None else np.clip(np.asarray(lens), 0, nk)
    ln = np.repeat(lens, group)[:, None, None]                                   # K/V slab s // group serves query slab s
    s = scale * np.einsum("bid,bjd->bij", q, np.repeat(k, group, axis=0))
    j, i = np.arange(nk)[None, None, :], np.arange(nq)[None, :, None]
    s = np.where((j < ln) & ((j <= ln - nq + i) if causal else True), s, -np.inf)  # bottom-right aligned diagonal
    m = s.max(axis=-1, keepdims=True)
    p = np.exp(s - np.where(np.isfinite(m), m, 0.0))                              # a row without keys: all zeros
    l = p.sum(axis=-1, keepdims=True)
    o = np.einsum("bij,bjd->bid", p, np.repeat(v, group, axis=0)) / np.where(l > 0, l, 1.0)
    with np.errstate(divide="ignore"):
        return o, (np.where(np.isfinite(m), m, 0.0) + np.log(l))[..., 0]
