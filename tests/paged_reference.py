"""Reference side of the paged KV-cache forward (include/flashattn_amd_paged.h): rebuild the contiguous cache a block table describes.  The
reference RESULT is tests/kv_reference.attention_kv on the gathered cache; tests/test_paged_host.py pins gather() on a hand-written example."""
import numpy as np


def gather(pool, table, lens, nk=None):
    """pool (pages, page, d) or (pages, page, H, d); table (batch, max_pages) of physical page numbers; lens: keys per sequence.
    Returns (batch * H, nk, d), nk = max(lens) unless given: row j of slab b * H + h is pool[table[b][j // page], j % page, h] for j < lens[b]
    and zero from there on.  Only what the contract lets a forward read is touched: table entries below ceil(len / page), rows below len."""
    pool, table = np.asarray(pool), np.asarray(table)
    if pool.ndim == 3:
        pool = pool[:, :, None, :]
    page, H, d = pool.shape[1:]
    lens = [int(n) for n in lens]
    assert len(lens) == table.shape[0]
    nk = max(lens + [1]) if nk is None else int(nk)
    out = np.zeros((table.shape[0] * H, nk, d), dtype=pool.dtype)
    for b, n in enumerate(lens):
        n = min(n, nk)
        for p in range(-(-n // page)):
            rows = min(page, n - p * page)
            phys = int(table[b, p])
            assert 0 <= phys < pool.shape[0], (b, p, phys)
            out[b * H:(b + 1) * H, p * page:p * page + rows] = pool[phys, :rows].transpose(1, 0, 2)
    return out
